"""Host-side mirror of the reference's `ParallelWavenet` for the generation path.

Same constructor argument (the hparams Namespace), same `feed_forward({'mel': ...})`
result keys and `_clip_quant_scale` as wavenet/parallel_wavenet.py:117-141,289-359 of
the reference -- but `feed_forward` is ONE call into the HIP engine instead of a TF
graph.  The reference creates TF variables and a Saver restores them; here
`restore(checkpoint_path)` / `load_weights(dict)` fills the engine.

With a teacher (the mirror's `Wavenet`, passed as `teacher=` like the reference's), the student is scored against it:
`kl_loss_logistic`, `kl_loss_gauss`, `power_loss`, `contrastive_loss` and `calculate_loss` (parallel_wavenet.py:361-512)
take the reference's keys and return the reference's dicts, as 0-d float64 device tensors.  The teacher's full-sequence
forward runs on the student's unclipped x (CLIP = False) and the loss kernels of csrc/wn_distill.hip score it; the
Monte-Carlo draws are injected (`noise`, [B, num_samples, T]) or drawn on the device from `seed`.

The losses are differentiable with respect to the student's 'x', 'mean_tot' and 'scale_tot' (DESIGN.md 12): when grad mode is
on and one of them requires grad, they are composed of the autograd Functions of distill_autograd.py -- the same kernels
for the values (the same bits), the gradient kernels and the teacher's input VJP for `backward()`.  Otherwise they take the
plain path (no tape).  H_Ps is computed from scale_tot, so its gradient goes to scale_tot: 1 / (N scale_tot), which is the
reference's gradient through log_scale_tot wherever scale_tot = exp(log_scale_tot).

Without a teacher: `encode` / `log_prob` give the student's own likelihood of real audio, and
`nll_and_weight_grads` its gradient with respect to the student's variables, the audio and the encoding --
the loss of maximum-likelihood training (train.StudentMleTrainer).
"""
import numpy as np
import torch

from .. import config as cfg
from ..engine import Engine, NotConverged
from .. import distill_autograd as dag


def _req(d, k):
    return isinstance(d.get(k), torch.Tensor) and d[k].requires_grad


def _wants_grad(d, keys=('x', 'mean_tot', 'scale_tot')):
    return torch.is_grad_enabled() and any(_req(d, k) for k in keys)


def _grad_inputs(te, ff_dict):
    """the teacher's out_params (through its tape when x requires grad) and mean_tot / scale_tot as tensors"""
    x = ff_dict['x']
    out_params = dag.TeacherForward.apply(x, ff_dict['mel'], te) if _req(ff_dict, 'x') else te.teacher_forward(x, ff_dict['mel'])
    mean, scale = (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float32), device=te.device)
                   for v in (ff_dict['mean_tot'], ff_dict['scale_tot']))
    return out_params, mean, scale


class ParallelWavenet(object):
    def __init__(self, hparams, teacher=None, train_path=None, device=None):
        self.hparams = cfg.load_hparams(hparams)
        hp = self.hparams
        self.use_mu_law = hp.use_mu_law
        self.use_weight_norm = getattr(hp, 'use_weight_norm', False)
        self.use_resize_conv = getattr(hp, 'use_resize_conv', False)
        self.upsample_act = getattr(hp, 'upsample_act', 'tanh')
        self.loss_type = getattr(hp, 'loss_type', 'logistic')
        self.use_share_deconv = getattr(hp, 'use_share_deconv', False)
        self.use_teacher_deconv = getattr(hp, 'use_teacher_deconv', False)
        assert not (self.use_share_deconv and self.use_teacher_deconv)
        self.quant_chann = 2 ** 8 if self.use_mu_law else 2 ** 16
        self.out_width = 2
        self.engine = Engine(hp, kind='student', device=device)
        # the teacher scores the student in the distillation losses below; generation needs none.  The pairing the
        # reference asserts at construction (parallel_wavenet.py:129-136) is checked where a loss uses the teacher.
        self.teacher = teacher

    def load_weights(self, weights):
        self.engine.load_weights(weights)
        return self

    def restore(self, checkpoint_path):
        self.engine.load_checkpoint(checkpoint_path)
        return self

    def feed_forward(self, inputs, init=False, noise=None, seed=0):
        """inputs: {'mel': [B,F,80]} (numpy or torch).  Returns device tensors
        x, mean_tot, scale_tot, log_scale_tot, rand_input, each [B,T].
        `noise` injects the logistic/normal draws (the reference draws them inside
        the graph, unseeded); `seed` drives the on-device Philox generator otherwise.
        When grad mode is on and inputs['mel'] or `noise` is a tensor that requires grad, x, mean_tot and scale_tot come
        from the tape forward instead (Engine.iaf_forward_train_tape: the values loss_and_weight_grads differentiates)
        and carry a gradient to those inputs; a drawn noise (noise=None) gets none.  The tape forward's
        refusals (mu-law, weight norm, a width that is no multiple of 64) surface as they are."""
        if torch.is_grad_enabled() and (_req(inputs, 'mel') or _req({'noise': noise}, 'noise')):
            return self._feed_forward_grad(inputs['mel'], noise, seed)
        out = self.engine.iaf_generate(inputs['mel'], noise=noise, seed=seed,
                                       want=('x', 'mean_tot', 'scale_tot', 'rand_input'))
        # log_scale_tot = min(sum_k log scale_k, 7) == log(min(prod_k scale_k, e^7)): a derived
        # diagnostic the generation path never consumes (only the training losses do).
        out['log_scale_tot'] = torch.log(out['scale_tot'])
        return {k: out[k] for k in ('x', 'mean_tot', 'scale_tot', 'log_scale_tot', 'rand_input')}

    def _input_grad_stacks(self):
        """[(engine, scope)] that differentiates each slice of d_encoding with respect to mel.  A teacher-owned stack
        (use_teacher_deconv) goes to the teacher's handle; without a teacher object, to this handle's copy of the same
        variables ('iaf_share')."""
        eng = self.engine
        if self.use_teacher_deconv:
            return [(self.teacher.engine, '')] if self.teacher is not None else [(eng, 'iaf_share')]
        return [(eng, scope) for scope in eng.iaf_stack_scopes()]

    def _feed_forward_grad(self, mel, noise, seed):
        eng = self.engine
        mel = eng._dev(mel)           # differentiable for a tensor: the gradient returns to the caller's device and dtype
        if noise is None:
            noise = eng.iaf_generate(mel.detach(), seed=seed, want=('rand_input',), check_range=False)['rand_input']
        noise = eng._dev(noise)
        x, mean_tot, scale_tot = dag.IafFeedForward.apply(mel, noise, eng, self._input_grad_stacks())
        return {'x': x, 'mean_tot': mean_tot, 'scale_tot': scale_tot, 'log_scale_tot': torch.log(scale_tot),
                'rand_input': noise.detach()}

    def encode(self, inputs, **kw):
        """The inverse of feed_forward.  inputs: 'mel' [B,F,80] and the audio as 'x' (feed_forward's key)
        or 'wav' [B,T], T = the student's length for F frames.  Returns z with feed_forward(noise=z)['x'] == x,
        log_scale_tot, log_probs (log p(x[t]) under the student), sweeps and converged ([B] bool).  Keyword arguments go
        to Engine.iaf_encode (z_init, max_sweeps, tol, check_every, z_max)."""
        x = inputs['x'] if 'x' in inputs else inputs['wav']
        r = self.engine.iaf_encode(x, inputs['mel'], want=('z', 'scale_tot', 'log_prob'), **kw)
        return {'z': r['z'], 'log_scale_tot': torch.log(r['scale_tot']), 'log_probs': r['log_prob'],
                'log_prob_sums': r['log_prob_sums'], 'sweeps': r['sweeps'], 'converged': r['converged']}

    def log_prob(self, inputs, adjoint_tol=None, **kw):
        """The student's log-likelihood of real audio: {'log_probs': [B,T], 'loss': -mean log p} (a 0-d float64 device
        tensor, from the kernel's float64 row sums).  Needs no teacher.  Raises when a row did not converge.
        When grad mode is on and inputs['mel'] or the audio is a tensor that requires grad, both results carry a gradient to
        them: the values are the same bits -- the encode runs as it does without grad -- and backward() runs
        the tape forward at z, the adjoint solve (Engine.iaf_adjoint, tolerance `adjoint_tol`) and, for mel, one
        Engine.deconv_backward_input per stack; it raises when the adjoint did not converge.  The student's weights get
        their gradient from nll_and_weight_grads."""
        key = 'x' if 'x' in inputs else 'wav'
        if torch.is_grad_enabled() and (_req(inputs, 'mel') or _req(inputs, key)):
            return self._log_prob_grad(inputs[key], inputs['mel'], adjoint_tol, kw)
        r = self.encode(inputs, **kw)
        if not bool(r['converged'].all()):
            raise NotConverged('log_prob: the inverse did not converge in {} sweeps'.format(r['sweeps']))
        return {'log_probs': r['log_probs'], 'loss': -(r['log_prob_sums'].sum() / r['log_probs'].numel())}

    def _log_prob_grad(self, wav, mel, adjoint_tol, kw):
        eng = self.engine
        wav, mel = eng._dev(wav), eng._dev(mel)          # differentiable for tensors: the gradients return to the caller's
        enc = eng.iaf_encode(wav.detach(), mel.detach(), want=('z', 'log_prob'), **kw)
        if not bool(enc['converged'].all()):
            raise NotConverged('log_prob: the inverse did not converge in {} sweeps'.format(enc['sweeps']))
        adj = {'adjoint_tol': adjoint_tol, 'check_every': kw.get('check_every', 8)}
        lp, sums = dag.IafLogProb.apply(wav, mel, eng, self._input_grad_stacks(), enc, adj)
        return {'log_probs': lp, 'loss': -(sums.sum() / lp.numel())}

    def nll_and_weight_grads(self, inputs, upsampler=True, encode_tol=1e-5, adjoint_tol=None, **kw):
        """-mean log p(wav | mel) under the student and its gradient with respect to the student's own variables, the audio
        and the encoding: maximum-likelihood training on real audio, no teacher.  inputs: 'mel' [B,F,80] and
        'wav' [B,T']; a wav longer than T = the student's length for F frames is centre-cropped as power_loss crops it, a
        shorter one is refused.  One encode (Engine.iaf_encode with tol = encode_tol; further keyword arguments go there),
        one tape forward at z, the adjoint solve (Engine.iaf_adjoint, tolerance adjoint_tol; max_sweeps and check_every bound
        and pace it as they do the encode), one reverse pass over the tape
        (Engine.iaf_backward_weights).  Raises when the encode or the adjoint did not converge.
        Returns 'loss' and 'log_probs' -- the bits of log_prob(inputs, tol=encode_tol) -- 'grads', 'flat_grads', 'd_encoding'
        and, with upsampler=True, the deconv stacks' entries and 'flat_upsampler_grads', laid out as loss_and_weight_grads
        lays them out; 'd_wav' [B,T] (of the cropped audio), 'sweeps' and 'adjoint_sweeps' (int) and 'converged' ([B] bool)."""
        from ..engine import _trim
        eng = self.engine
        mel = eng._dev(inputs['mel']).detach()
        wav = eng._dev(inputs['wav']).detach()
        T = eng.iaf_length(int(mel.shape[1])) if mel.dim() == 3 else 0
        if wav.dim() != 2 or int(wav.shape[1]) < T:
            raise ValueError('nll_and_weight_grads: wav must be [B, >= {}] for {} mel frames, got {}'.format(
                T, int(mel.shape[1]) if mel.dim() == 3 else '?', tuple(wav.shape)))
        if int(wav.shape[1]) > T:
            wav = _trim(wav, int(wav.shape[1]) - T).contiguous()
        enc = eng.iaf_encode(wav, mel, want=('z', 'log_prob'), tol=encode_tol, **kw)
        if not bool(enc['converged'].all()):
            raise NotConverged('nll_and_weight_grads: the inverse did not converge in {} sweeps'.format(enc['sweeps']))
        lp, n = enc['log_prob'], enc['log_prob'].numel()
        # the cotangent of log p under -mean, as autograd hands it to IafLogProb.backward: the same bits on both roads
        c = torch.full(tuple(lp.shape), -1.0 / n, dtype=torch.float64, device=lp.device).to(torch.float32)
        a = dag.iaf_log_prob_adjoint(eng, mel, enc['z'], c, adjoint_tol=adjoint_tol, max_sweeps=kw.get('max_sweeps'),
                                     check_every=kw.get('check_every', 8))
        res = eng.iaf_backward_weights(a['tape'], -a['lam'], torch.zeros_like(a['lam']), a['d_scale_tot'], want_encoding=True)
        ret = {'loss': -(enc['log_prob_sums'].sum() / n), 'log_probs': lp, 'grads': res['grads'], 'flat_grads': res['flat_grads'],
               'd_encoding': res['d_encoding'], 'd_wav': a['lam'], 'sweeps': enc['sweeps'], 'adjoint_sweeps': a['sweeps'],
               'converged': enc['converged'] & a['converged']}
        if upsampler and not self.use_teacher_deconv:
            ret['grads'] = dict(res['grads'])
            ret['flat_upsampler_grads'] = {}
            for s, scope in enumerate(eng.iaf_stack_scopes()):
                up = eng.deconv_backward(mel, res['d_encoding'][s], scope)
                ret['grads'].update(up['grads'])
                ret['flat_upsampler_grads'][scope] = up['flat_grads']
        return ret

    def _clip_quant_scale(self, x, quant_chann=None, use_mu_law=None):
        wav, _ = self.engine.clip_quant(x)
        return wav

    # ---- distillation losses (parallel_wavenet.py:361-512) ----
    def _need_teacher(self, what):
        if self.teacher is None:
            raise ValueError('{} needs the teacher: ParallelWavenet(hparams, teacher=Wavenet(te_hparams))'.format(what))
        te = self.teacher
        if not (te.loss_type == 'mol' and self.loss_type == 'logistic' or te.loss_type == 'gauss' and self.loss_type == 'gauss'):
            raise ValueError('{}: a {} student is distilled from a {} teacher; the reference pairs logistic with mol and gauss '
                             'with gauss (parallel_wavenet.py:133-135)'.format(what, self.loss_type, te.loss_type))
        if self.use_mu_law:
            raise ValueError('{}: mu-law students are not supported by the distillation losses (the reference would '
                             'score mu-law encoded audio unencoded, CLIP = False)'.format(what))
        return self.teacher.engine

    def kl_loss_logistic(self, ff_dict, num_samples=100, noise=None, seed=0):
        """parallel_wavenet.py:361-402.  ff_dict: 'mel', 'x', 'mean_tot', 'scale_tot' (and 'log_scale_tot', which is
        log(scale_tot) here: H_Ps comes from the kernel's sum of log scale_tot).  Returns kl_loss, H_Ps, H_Ps_Pt."""
        te = self._need_teacher('kl_loss_logistic')
        if _wants_grad(ff_dict):
            out_params, mean, scale = _grad_inputs(te, ff_dict)
            sums = dag.MolXentSums.apply(out_params, mean, scale, te, num_samples, noise, seed)
            n = mean.numel()
            H_Ps = sums[1] / n + 2
            H_Ps_Pt = sums[0] / n
            return {'kl_loss': H_Ps_Pt - H_Ps, 'H_Ps': H_Ps, 'H_Ps_Pt': H_Ps_Pt}
        out_params = te.teacher_forward(ff_dict['x'], ff_dict['mel'])
        r = te.distill_mol_xent(out_params, ff_dict['mean_tot'], ff_dict['scale_tot'], num_samples, noise=noise, seed=seed)
        n = r['H_bl'].numel()
        H_Ps = r['sums'][1] / n + 2
        H_Ps_Pt = r['sums'][0] / n
        return {'kl_loss': H_Ps_Pt - H_Ps, 'H_Ps': H_Ps, 'H_Ps_Pt': H_Ps_Pt}

    def kl_loss_gauss(self, ff_dict):
        """parallel_wavenet.py:404-429: mean closed-form KL + 4 * mean squared log-scale difference."""
        te = self._need_teacher('kl_loss_gauss')
        if _wants_grad(ff_dict):
            out_params, mean, scale = _grad_inputs(te, ff_dict)
            sums = dag.GaussKLSums.apply(out_params, mean, scale, te)
            n = mean.numel()
            return {'kl_loss': sums[0] / n + 4.0 * (sums[1] / n)}
        out_params = te.teacher_forward(ff_dict['x'], ff_dict['mel'])
        r = te.distill_gauss_kl(out_params, ff_dict['mean_tot'], ff_dict['scale_tot'])
        n = r['kl_bl'].numel()
        return {'kl_loss': r['sums'][0] / n + 4.0 * (r['sums'][1] / n)}

    def power_loss(self, wav_dict):
        """parallel_wavenet.py:459-479: STFT-magnitude loss of 'x' against the real audio 'wav'."""
        from ..engine import power_loss
        if _wants_grad(wav_dict, ('x',)):
            return {'power_loss': dag.power_loss(wav_dict['x'], wav_dict['wav'])}
        return {'power_loss': power_loss(wav_dict['x'], wav_dict['wav'], device=self.engine.device)}

    def contrastive_loss(self, ff_dict, num_samples=100, noise=None, seed=0):
        """parallel_wavenet.py:481-490: minus the logistic KL under the mismatched 'mel_rand'."""
        ff_dict_for_cl = {'x': ff_dict['x'], 'mel': ff_dict['mel_rand'], 'mean_tot': ff_dict['mean_tot'],
                          'scale_tot': ff_dict['scale_tot'], 'log_scale_tot': ff_dict.get('log_scale_tot')}
        return {'contrastive_loss': -self.kl_loss_logistic(ff_dict_for_cl, num_samples, noise=noise, seed=seed)['kl_loss']}

    def calculate_loss(self, ff_dict, noise=None, seed=0, cl_noise=None, cl_seed=None):
        """parallel_wavenet.py:492-512 with the same hparams reads (power_loss_factor; for a logistic student num_samples and
        contrastive_loss_factor, with the reference's getattr defaults).  The contrastive term has draws of its own, like
        the reference's second random node: `cl_noise`, or the device generator under `cl_seed` (default: derived from
        `seed`, distinct from the KL term's stream)."""
        hp = self.hparams
        plf = hp.power_loss_factor
        if self.loss_type == 'logistic':
            clf = getattr(hp, 'contrastive_loss_factor', 0.0)
            num_samples = getattr(hp, 'num_samples', 0)
            loss_dict = self.kl_loss_logistic(ff_dict, num_samples, noise=noise, seed=seed)
        else:
            clf = 0.
            num_samples = 0
            loss_dict = self.kl_loss_gauss(ff_dict)
        loss = loss_dict['kl_loss']
        if plf > 0.0:
            pl_dict = self.power_loss(ff_dict)
            loss = loss + plf * pl_dict['power_loss']
            loss_dict.update(pl_dict)
        if clf > 0.0:
            if cl_seed is None:
                cl_seed = (int(seed) + 0x9E3779B97F4A7C15) % (1 << 64)
            cl_dict = self.contrastive_loss(ff_dict, num_samples, noise=cl_noise, seed=cl_seed)
            loss = loss + clf * cl_dict['contrastive_loss']
            loss_dict.update(cl_dict)
        loss_dict.update({'loss': loss})
        return loss_dict

    def loss_and_weight_grads(self, inputs, seed=0, noise=None, upsampler=True):
        """The loss train_parallel_wavenet.py minimises and its gradient with respect to the student's own variables
        (DESIGN.md 19).  inputs: 'mel' [B,F,80] and 'wav' [B,T'], plus 'mel_rand' where contrastive_loss_factor > 0.
        `noise` [B,T] injects the student's draw (None: the device generator under `seed`); `seed` also drives the
        Monte-Carlo draws of calculate_loss, as in calculate_loss(feed_forward(inputs, seed=seed), seed=seed).
        One tape forward (Engine.iaf_forward_train_tape), calculate_loss on its x, mean_tot and scale_tot as leaves,
        backward() through the frozen teacher, one reverse pass over the tape (Engine.iaf_backward_weights).
        Returns calculate_loss's dict -- the bits of the no-grad calculate_loss on the same forward values -- plus
        'grads': {tf variable name: d loss / d variable in the TF shape}, 'flat_grads' (Engine.iaf_grad_table gives the
        offsets) and 'd_encoding' [n_stacks, B, F frame_shift, deconv_width].
        upsampler=True: 'grads' also holds '<scope>/trans_conv_j/kernel' and '/bias' of every deconv stack the student owns
        ('iaf_share', or 'iaf_k' per flow), from one Engine.deconv_backward per stack on this call's d_encoding, and
        'flat_upsampler_grads' maps the scope to that call's flat vector.  With use_teacher_deconv the encoding is the
        teacher's and is not trained: the step is skipped.  The teacher stays frozen; the optimiser is the caller's."""
        eng = self.engine
        mel = eng._dev(inputs['mel'])
        ff, tape = eng.iaf_forward_train_tape(mel, noise=noise, seed=seed)
        leaves = {k: ff[k].detach().requires_grad_(True) for k in ('x', 'mean_tot', 'scale_tot')}
        ff_dict = dict(leaves, mel=mel, wav=inputs['wav'], rand_input=ff['rand_input'])
        if 'mel_rand' in inputs:
            ff_dict['mel_rand'] = inputs['mel_rand']
        with torch.enable_grad():
            loss_dict = self.calculate_loss(ff_dict, seed=seed)
            loss_dict['loss'].backward()
        cot = [v.grad if v.grad is not None else torch.zeros_like(v) for v in (leaves['x'], leaves['mean_tot'], leaves['scale_tot'])]
        res = eng.iaf_backward_weights(tape, cot[0], cot[1], cot[2], want_encoding=True)
        ret = {k: v.detach() for k, v in loss_dict.items()}
        ret.update({'grads': res['grads'], 'flat_grads': res['flat_grads'], 'd_encoding': res['d_encoding']})
        if upsampler and not self.use_teacher_deconv:
            scopes = ['iaf_share'] if self.use_share_deconv else ['iaf_{:d}'.format(k + 1) for k in range(eng.iaf_n_stacks())]
            ret['grads'] = dict(res['grads'])
            ret['flat_upsampler_grads'] = {}
            for s, scope in enumerate(scopes):
                up = eng.deconv_backward(mel, res['d_encoding'][s], scope)
                ret['grads'].update(up['grads'])
                ret['flat_upsampler_grads'][scope] = up['flat_grads']
        return ret
