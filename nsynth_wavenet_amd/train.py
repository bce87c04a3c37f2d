"""Training the teacher on the device: train_wavenet.py's AdamOptimizer(lr, epsilon=1e-8), its optional
clip_by_global_norm and its ExponentialMovingAverage(0.9999, num_updates=global_step) on top of
Wavenet.loss_and_weight_grads, with the updated weights re-packed into the SAME handle by Engine.teacher_set_weights.  No
weight and no gradient crosses to the host during a step.

    teacher = Wavenet(hparams).load_weights(w)
    trainer = TeacherTrainer(teacher, w, lr={0: 2e-4, 90000: 6e-5})
    for batch in batches:                       # {'wav': [B,T], 'mel': [B,F,80]}
        out = trainer.step(batch)               # {'loss', 'log_probs', 'grad_norm'}: device tensors
    np.savez('eval.npz', **trainer.weights(ema=True))
"""
import math

import numpy as np
import torch

from .engine import adam_ema_step, grad_sumsq


def scheduled_lr(lr, global_step):
    """The learning rate train_wavenet.py:141-144 builds from a {step: lr} dict (wavenet.py:100): schedule[0], replaced in
    the dict's own order by every entry whose key is <= global_step.  A float is a constant rate."""
    if not isinstance(lr, dict):
        return float(lr)
    if 0 not in lr:
        raise ValueError('an lr schedule needs an entry for step 0 (train_wavenet.py:141)')
    cur = lr[0]
    for key, value in lr.items():
        if not global_step < key:
            cur = value
    return float(cur)


class TeacherTrainer(object):
    """One teacher handle trained step after step.

    wavenet:  a loaded Wavenet (MoL or Gauss, no mu-law, no weight norm; a resize-conv upsampler needs upsampler=False).
    weights:  the dict it was loaded from -- the handle keeps no host copy, and the packs do not give the values back exactly.
    lr:       a float or a {step: lr} schedule keyed by the number of completed steps (scheduled_lr).
    clip_norm: None, or the bound of tf.clip_by_global_norm over all trained variables.
    upsampler: also train trans_conv_j/kernel and /bias; with False the upsampler keeps its weights.

    Order inside a step (the reference's tf.group leaves it open): Adam first, with t = completed steps + 1; then the EMA of
    the UPDATED weights with num_updates = the number of steps completed BEFORE this one, i.e. the decay of step 1 is
    min(ema_decay, 1 / 10).  The shadows start equal to the weights."""

    def __init__(self, wavenet, weights, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.9999, clip_norm=None,
                 upsampler=True):
        self.net = wavenet
        self.eng = eng = wavenet.engine
        self.lr, self.beta1, self.beta2, self.eps = lr, float(beta1), float(beta2), float(eps)
        self.ema_decay = float(ema_decay)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.upsampler = bool(upsampler)
        scheduled_lr(lr, 0)
        self.tables = [eng.teacher_grad_table()]
        if self.upsampler:
            self.tables.append(eng.deconv_grad_table(''))
        if not all(self.tables):
            raise ValueError('TeacherTrainer: this model has no weight gradients on the device (mu-law, ce, weight norm or '
                             'a resize-conv upsampler with upsampler=True)')
        dev = eng.device
        self.p, self.m, self.v, self.ema = [], [], [], []
        sizes = [eng.teacher_grad_floats()] + ([eng.deconv_grad_floats('')] if self.upsampler else [])
        for tab, size in zip(self.tables, sizes):
            flat = np.zeros(size, np.float32)        # the library's own count; anything a table does not cover stays zero
            for name, off, shape in tab:
                a = np.asarray(weights[name], np.float32)
                if a.size != int(np.prod(shape)):
                    raise ValueError('TeacherTrainer: {} has {} values, the model expects shape {}'.format(name, a.size, shape))
                flat[off:off + a.size] = a.reshape(-1)          # Saver(reshape=True): same element count
            p = torch.from_numpy(flat).to(dev)
            self.p.append(p)
            self.m.append(torch.zeros_like(p))
            self.v.append(torch.zeros_like(p))
            self.ema.append(p.clone())
        trained = set(name for tab in self.tables for name, _, _ in tab)
        self._frozen = {k: np.array(a, np.float32) for k, a in weights.items() if k not in trained}   # upsampler=False
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.global_step = 0              # completed steps
        self.lr_t = None                  # the bias-corrected rate of the last step, as handed to the kernel (float32)
        self.lr_history = []              # the scheduled rate of every step

    def _grads(self, inputs):
        out = self.net.loss_and_weight_grads(inputs, upsampler=self.upsampler)
        flats = [out['flat_grads']]
        if self.upsampler:
            flats.append(out['flat_upsampler_grads'])
        return out, flats

    def _update(self, flats):
        """grad_sumsq over both buffers and adam_ema_step on both; returns the global norm (0-d float64 device tensor)"""
        n, t = self.global_step, self.global_step + 1
        lr = scheduled_lr(self.lr, n)
        self.lr_history.append(lr)
        self.lr_t = float(np.float32(lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)))
        decay_t = min(self.ema_decay, (1.0 + n) / (10.0 + n))
        for i, g in enumerate(flats):
            grad_sumsq(g, self.sumsq, accumulate=i > 0)
        for p, g, m, v, e in zip(self.p, flats, self.m, self.v, self.ema):
            adam_ema_step(p, g, m, v, e, self.lr_t, self.beta1, self.beta2, self.eps, decay_t,
                          sumsq=self.sumsq if self.clip_norm is not None else None,
                          clip_norm=self.clip_norm if self.clip_norm is not None else 1.0)
        return self.sumsq.sqrt()[0]

    def _repack(self, bufs):
        self.eng.teacher_set_weights(bufs[0], bufs[1] if self.upsampler else None)

    def step(self, inputs):
        """One training step on {'wav': [B,T], 'mel': [B,F,80]} -> {'loss': the loss BEFORE the update (the bits of
        calculate_loss(feed_forward(.)) under the weights in force at entry), 'log_probs': [B,T], 'grad_norm': the global
        norm of the gradient before clipping}, all device tensors."""
        out, flats = self._grads(inputs)
        norm = self._update(flats)
        self._repack(self.p)
        self.global_step += 1
        return {'loss': out['loss'], 'log_probs': out['log_probs'], 'grad_norm': norm}

    def weights(self, ema=False):
        """{tf name: numpy array in the TF shape} of every variable of the model: the weights, or with ema=True the shadow
        values under the plain names (what make_eval_model.py writes), for load_weights or an .npz for restore.  Variables that
        are not trained (the upsampler's with upsampler=False) come back as they were given."""
        out = {k: a.copy() for k, a in self._frozen.items()}
        for tab, buf in zip(self.tables, self.ema if ema else self.p):
            host = buf.cpu().numpy()
            for name, off, shape in tab:
                out[name] = host[off:off + int(np.prod(shape))].reshape(shape).copy()
        return out

    def use_ema(self):
        """Pack the shadow values into the handle, for generation after training (use_weights() puts the weights back)."""
        self._repack(self.ema)
        return self

    def use_weights(self):
        self._repack(self.p)
        return self
