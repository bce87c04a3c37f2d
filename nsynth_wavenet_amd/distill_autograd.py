"""torch.autograd Functions of the distillation losses.

Each forward calls the HIP kernels the no-grad loss path calls (so the values are the same bits) and each backward the
gradient kernels of csrc/wn_teacher_bwd.hip / wn_distill.hip.  The loss Functions return the raw float64 sums of their kernels;
the scalar arithmetic of the losses stays in torch, so a backward receives d loss / d sums as a device tensor and hands it
to the kernels without a host read.  The teacher is frozen: TeacherForward differentiates with respect to the audio only.
"""
import torch

from . import engine as _engine


class TeacherForward(torch.autograd.Function):
    """wav [B,T] -> out_params [B,T,out_width] of a teacher Engine; holds the tape of wn_teacher_forward_tape."""

    @staticmethod
    def forward(ctx, wav, mel, eng):
        out, tape = eng.teacher_forward_tape(wav.detach(), mel)
        ctx.eng, ctx.tape = eng, tape
        return out

    @staticmethod
    def backward(ctx, g):
        dwav = ctx.eng.teacher_backward_input(ctx.tape, g)
        ctx.tape = None
        return dwav, None, None


class IafFeedForward(torch.autograd.Function):
    """(mel [B,F,n_mel], noise [B,T]) -> (x, mean_tot, scale_tot) of a student Engine's tape forward;
    differentiable in both inputs.  The student is frozen here: its weights get their gradients from
    ParallelWavenet.loss_and_weight_grads.  stacks: [(engine, scope)] per slice of d_encoding, in the order of
    Engine.iaf_stack_scopes() -- a teacher-owned stack is differentiated under the teacher's handle."""

    @staticmethod
    def forward(ctx, mel, noise, eng, stacks):
        mel, noise = eng._dev(mel.detach()), eng._dev(noise.detach())
        ff, tape = eng.iaf_forward_train_tape(mel, noise=noise)
        ctx.eng, ctx.tape, ctx.stacks, ctx.mel = eng, tape, stacks, mel
        return ff['x'], ff['mean_tot'], ff['scale_tot']

    @staticmethod
    def backward(ctx, d_x, d_mean_tot, d_scale_tot):
        want_mel = ctx.needs_input_grad[0]
        res = ctx.eng.iaf_backward_input(ctx.tape, d_x, d_mean_tot, d_scale_tot, want_encoding=want_mel)
        d_mel = None
        if want_mel:
            for s, (eng, scope) in enumerate(ctx.stacks):
                g = eng.deconv_backward_input(ctx.mel, res['d_encoding'][s], scope)
                d_mel = g if d_mel is None else d_mel + g
        ctx.tape = None
        return d_mel, res['d_noise'] if ctx.needs_input_grad[1] else None, None, None


def iaf_log_prob_adjoint(eng, mel, z, d_log_prob, adjoint_tol=None, max_sweeps=None, check_every=8):
    """What every gradient of the student's log-likelihood starts from: the tape forward at noise = z, the
    cotangents of wn_iaf_latent_log_prob_grad on the tape's scale_tot, and the adjoint solve.  d_log_prob [B,T] float32.
    -> {'tape', 'lam' (= d / d x), 'd_scale_tot', 'sweeps', 'converged'}; the weights and the encoding take theirs from
    iaf_backward_weights / iaf_backward_input(tape, -lam, 0, d_scale_tot).  Raises when the solve did not converge."""
    ff, tape = eng.iaf_forward_train_tape(mel, noise=z)
    g_z, d_s = eng.iaf_latent_log_prob_grad(z, ff['scale_tot'], d_log_prob)
    r = eng.iaf_adjoint(tape, g_z, d_s, tol=eng.ADJOINT_TOL if adjoint_tol is None else adjoint_tol, max_sweeps=max_sweeps,
                        check_every=check_every)
    if r['replaced'] or not bool(r['converged'].all()):
        raise _engine.NotConverged('log_prob: the adjoint of the inverse did not converge in {} sweeps (max |update| / max |lam| = '
                                   '{:.3g}, {} non-finite values)'.format(r['sweeps'], float((r['resid'][:, 0] / r['resid'][:, 1]).max()),
                                                                          r['replaced']))
    return {'tape': tape, 'lam': r['lam'], 'd_scale_tot': d_s, 'sweeps': r['sweeps'], 'converged': r['converged']}


class IafLogProb(torch.autograd.Function):
    """(wav [B,T], mel [B,F,n_mel]) -> (log_probs [B,T], log_prob_sums [B] float64) of a student Engine: the values an encode
    already computed (`enc`: Engine.iaf_encode's 'z', 'log_prob', 'log_prob_sums'), handed on unchanged; differentiable in
    both inputs by the adjoint of the inverse.  stacks: as for IafFeedForward.  adj: keyword arguments of
    iaf_log_prob_adjoint."""

    @staticmethod
    def forward(ctx, wav, mel, eng, stacks, enc, adj):
        ctx.eng, ctx.stacks, ctx.adj = eng, stacks, adj
        ctx.mel, ctx.z = eng._dev(mel.detach()), enc['z']
        return enc['log_prob'].clone(), enc['log_prob_sums'].clone()

    @staticmethod
    def backward(ctx, d_lp, d_sums):
        eng, z = ctx.eng, ctx.z
        c = d_sums.to(torch.float32)[:, None].expand_as(z)
        c = (c + d_lp if d_lp is not None else c).contiguous()
        a = iaf_log_prob_adjoint(eng, ctx.mel, z, c, **ctx.adj)
        d_mel = None
        if ctx.needs_input_grad[1]:
            zero = torch.zeros_like(a['lam'])
            res = eng.iaf_backward_input(a['tape'], -a['lam'], zero, a['d_scale_tot'], want_encoding=True)
            for s, (e, scope) in enumerate(ctx.stacks):
                g = e.deconv_backward_input(ctx.mel, res['d_encoding'][s], scope)
                d_mel = g if d_mel is None else d_mel + g
        return a['lam'] if ctx.needs_input_grad[0] else None, d_mel, None, None, None, None


class TeacherLogProb(torch.autograd.Function):
    """(out_params [B,T,out_width], wav [B,T]) -> log_probs [B,T] of a teacher Engine.  The gradient to wav is
    the one through the TARGET (zero for mu-law and ce teachers); the one through the network input is TeacherForward's."""

    @staticmethod
    def forward(ctx, out_params, wav, eng):
        out_params, wav = eng._dev(out_params.detach()), eng._dev(wav.detach())
        ctx.save_for_backward(out_params, wav)
        ctx.eng = eng
        return eng.teacher_log_prob(out_params, wav)

    @staticmethod
    def backward(ctx, g):
        out_params, wav = ctx.saved_tensors
        d_out, d_wav = ctx.eng.teacher_log_prob_grad(out_params, wav, g, want_wav=ctx.needs_input_grad[1])
        return d_out, d_wav, None


class MolXentSums(torch.autograd.Function):
    """(out_params, mean_tot, scale_tot) -> sums [2] of wn_distill_mol_xent: sum of H_bl, sum of log scale_tot."""

    @staticmethod
    def forward(ctx, out_params, mean_tot, scale_tot, eng, num_samples, noise, seed):
        r = eng.distill_mol_xent(out_params.detach(), mean_tot.detach(), scale_tot.detach(), num_samples, noise=noise,
                                 seed=seed)
        ctx.save_for_backward(out_params.detach(), mean_tot.detach(), scale_tot.detach())
        ctx.eng, ctx.S, ctx.noise, ctx.seed = eng, num_samples, noise, seed
        return r['sums']

    @staticmethod
    def backward(ctx, g):
        te, mean, scale = ctx.saved_tensors
        d_te, d_m, d_s = ctx.eng.distill_mol_xent_grad(te, mean, scale, ctx.S, g, noise=ctx.noise, seed=ctx.seed)
        return d_te, d_m, d_s, None, None, None, None


class GaussKLSums(torch.autograd.Function):
    """(out_params, mean_tot, scale_tot) -> sums [2] of wn_distill_gauss_kl: sum of kl_bl, sum of the squared log-scale
    differences."""

    @staticmethod
    def forward(ctx, out_params, mean_tot, scale_tot, eng):
        r = eng.distill_gauss_kl(out_params.detach(), mean_tot.detach(), scale_tot.detach())
        ctx.save_for_backward(out_params.detach(), mean_tot.detach(), scale_tot.detach())
        ctx.eng = eng
        return r['sums']

    @staticmethod
    def backward(ctx, g):
        te, mean, scale = ctx.saved_tensors
        d_te, d_m, d_s = ctx.eng.distill_gauss_kl_grad(te, mean, scale, g)
        return d_te, d_m, d_s, None


class PowerSums(torch.autograd.Function):
    """(pred, orig) [B,L] of equal length -> out2 [2] of wn_power_loss; differentiable in pred."""

    @staticmethod
    def forward(ctx, pred, orig):
        pred = pred.detach()
        ctx.save_for_backward(pred, orig)
        return _engine.power_loss_sums(pred, orig)

    @staticmethod
    def backward(ctx, g):
        pred, orig = ctx.saved_tensors
        return _engine.power_loss_grad(pred, orig, g), None


def power_loss(pred, orig):
    """engine.power_loss with a gradient to pred: the same trims, the same kernel and the same scalar arithmetic."""
    dev = pred.device
    orig = orig.to(device=dev, dtype=torch.float32) if isinstance(orig, torch.Tensor) else \
        torch.as_tensor(orig, dtype=torch.float32, device=dev)
    pred = pred.to(dtype=torch.float32)
    if pred.dim() != 2 or orig.dim() != 2 or pred.shape[0] != orig.shape[0]:
        raise ValueError('power_loss: pred and orig must be [B,L] with equal B')
    pred = pred if pred.stride(1) == 1 else pred.contiguous()
    orig = (orig if orig.stride(1) == 1 else orig.contiguous()).detach()
    lp, lo = int(pred.shape[1]), int(orig.shape[1])
    if lp > lo:
        pred = _engine._trim(pred, lp - lo)
    elif lo > lp:
        orig = _engine._trim(orig, lo - lp)
    B, L = int(pred.shape[0]), int(pred.shape[1])
    out = PowerSums.apply(pred, orig)
    nf = (L + _engine.STFT_HOP - 1) // _engine.STFT_HOP
    return 0.5 * out[0] / (B * nf * _engine.STFT_BINS) + 0.5 * out[1] / (B * nf * _engine.PRIORITY_FREQ)
