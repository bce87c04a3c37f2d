"""Engine: one model on one GPU behind the C ABI (include/wnhip.h).

PyTorch-ROCm is used only for device memory, streams and (in dist.py)
torch.distributed; every arithmetic operation of the generation path runs in the
hand-written HIP kernels of libwnhip.so.  There is no CPU or eager fallback: a
missing library or a missing GPU raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import config as cfg
from . import weights as wts


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class NotConverged(RuntimeError):
    """The inverse of the student (the encode's sweeps) or its adjoint did not converge within the sweeps it was given.
    A RuntimeError, as these refusals always were; a type of its own so that a caller that goes on after one -- the sharded
    maximum-likelihood step -- tells it from any other failure without reading the message."""


class Engine(object):
    """Replaces one TF graph + Session of the reference (parallelgen.py:24-41,
    fastgen.py:139-150): built from hparams, filled with named weights."""

    def __init__(self, hparams, kind=None, device=None, n_mel=80, precision=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError('nsynth_wavenet_amd needs a ROCm GPU: the generation path has no CPU fallback')
        self.hp = cfg.load_hparams(hparams)
        self.kind = kind or cfg.model_kind(self.hp)
        self.device = torch.device(device if device is not None else 'cuda:{}'.format(torch.cuda.current_device()))
        self.n_mel = n_mel
        self._hbox = [ctypes.c_void_p(0)]   # the C handle, shared with the engine's forks (fork())
        self._shared = {'ar_graph': None,   # handle-wide switch states the forks must agree on
                        'grad_tables': {}}  # (which, scope) -> the handle's gradient tables (_grad_table)
        self._is_fork = False
        self._ws = None
        self._ar_stream = None
        self._ar_groups = None              # per-group streams / queue states of ar_generate(streams=G)
        self._last_ws = None
        self._enc_ws = None               # iaf_encode's own workspace: the conditioning term lives there between its C calls
        self._train_frames = {}           # tape address -> mel frames of the training tapes written through this handle
        self.range_fallbacks = 0          # calls re-run on the fp32 form because they left the fp16 range
        self._finalized = False
        self.precision = precision or cfg.default_precision()
        c = cfg.to_wn_config(self.hp, self.kind, n_mel, self.precision)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.wn_create(ctypes.byref(c), ctypes.byref(self._hbox[0])))
        self.quant_chann = cfg.quant_chann(self.hp)
        self.frame_shift = cfg.frame_shift(self.hp)

    @property
    def _h(self):
        return self._hbox[0]

    # ---- lifecycle ----
    def close(self):
        """Destroy the C handle (the owner) / drop this caller's workspace (a fork: the handle belongs to its parent)."""
        self._ws = self._last_ws = self._enc_ws = None
        if self._is_fork:
            return
        if self._h:
            torch.cuda.synchronize(self.device)
            self.lib.wn_destroy(self._h)
            self._hbox[0] = ctypes.c_void_p(0)

    def fork(self):
        """A second CALLER of the same C handle (SURVEY 8(b) "Threading / streams": a finalized handle is immutable and
        may be shared by concurrent callers using distinct workspaces and streams): shares the packed weights on the
        device, owns its workspace, and issues its work on the torch stream that is current in the calling thread
        (`with torch.cuda.stream(s): fork.iaf_generate(...)`).  Forks are what host threads use -- one fork per thread;
        an Engine object itself (one workspace) is not to be shared between threads.  The parent must outlive its forks."""
        import copy
        if not self._finalized:
            raise RuntimeError('fork() needs a finalized engine (load_weights first)')
        f = copy.copy(self)                 # same _hbox / _shared objects, same hparams
        f._is_fork = True
        f._ws = f._last_ws = f._enc_ws = f._ar_stream = None
        f._ar_groups = None
        f.range_fallbacks = 0
        return f

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        _lib.check(rc, self._h)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- weights ----
    def set_weight(self, name, array):
        a = np.ascontiguousarray(np.asarray(array, np.float32))
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        self._check(self.lib.wn_set_weight(self._h, name.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                           shape, a.ndim))

    def load_weights(self, weights):
        """weights: dict TF-variable-name -> ndarray (see weights.expected_variables)."""
        for name, _ in wts.expected_variables(self.hp, self.kind, self.n_mel):
            if name not in weights:
                raise KeyError('missing variable {}'.format(name))
            self.set_weight(name, weights[name])
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_finalize(self._h))
        self._shared['grad_tables'].clear()
        self._finalized = True
        return self

    def load_checkpoint(self, path):
        return self.load_weights(wts.load_checkpoint(path, self.hp, self.kind))

    # ---- helpers ----
    def iaf_length(self, F):
        return int(self.lib.wn_iaf_length(self._h, int(F)))

    def ar_length(self, F):
        return int(self.lib.wn_ar_length(self._h, int(F)))

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            if self._ws is not None:
                self.check_range()        # asynchronous calls not yet asked about: their status words live in the old buffer
            self._ws = self._last_ws = None
            try:
                self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
                if self._ws.numel() >= 64:                 # the range-guard words at its head start from zero
                    with torch.cuda.device(self.device):
                        self._check(self.lib.wn_iaf_range_reset(self._h, _ptr(self._ws), self._stream()))
            except torch.cuda.OutOfMemoryError as e:
                raise MemoryError('workspace of {:.1f} GB does not fit on {} ({}); for the IAF path '
                                  "precision='f16x3-fused' needs no conditioning workspace, or split the batch"
                                  .format(nbytes / 1e9, self.device, str(e).splitlines()[0]))
        return self._ws

    def _dev(self, x, dtype=torch.float32):
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.device)

    # ---- IAF path ----
    def iaf_generate(self, mel, noise=None, seed=0, want=('wav',), check_range=True, form=None):
        """ParallelWavenet.feed_forward + _clip_quant_scale.  mel [B,F,n_mel].
        Returns a dict of device tensors for the names in `want` out of
        wav, idx, x, mean_tot, scale_tot, rand_input.

        check_range (default): the split-fp16 arithmetic carries activations with the fp16 exponent range; when a
        call leaves it (|activation| >= 65504, possible after flows with scales near e^7) the library NaN-poisons the
        outputs and raises a status word.  The engine then reads that word (one 4-byte read-back, which synchronises
        the stream) and transparently re-runs the call on the fp32-MFMA form, so the caller always gets the
        reference's fp32 behaviour; `self.range_fallbacks` counts those re-runs.  check_range=False keeps the call
        asynchronous (serving / timing loops): call check_range() afterwards -- it raises if ANY call since the last
        check overflowed (the library accumulates the status words in the workspace; each such call NaN-poisoned its
        own outputs).  form: one of _lib.FORM_* to name the arithmetic of the call (None: the engine's default), e.g. the
        form an iaf_encode reports."""
        mel = self._dev(mel)
        if mel.dim() != 3 or mel.shape[2] != self.n_mel:
            raise ValueError('mel must be [batch, frames, {}], got {}'.format(self.n_mel, tuple(mel.shape)))
        B, F = int(mel.shape[0]), int(mel.shape[1])
        T = self.iaf_length(F)
        noise = self._dev(noise)
        if noise is not None and tuple(noise.shape) != (B, T):
            raise ValueError('noise must be [{}, {}], got {}'.format(B, T, tuple(noise.shape)))
        out = self._window_outputs(B, T, want)
        with torch.cuda.device(self.device):
            form = _lib.FORM_DEFAULT if form is None else int(form)
            try:
                ws = self._workspace(self.lib.wn_workspace_bytes(self._h, B, F))
            except MemoryError:
                # the hoisted-conditioning workspace (17.5 KB per generated sample) does not fit beside what else lives
                # on this GPU: the fused form needs none of it
                if self.precision not in ('f16x3', 'f16x3-hoisted'):
                    raise
                form = _lib.FORM_F16X3_FUSED
                ws = self._workspace(self.lib.wn_iaf_workspace_bytes_form(self._h, form, B, F))

            def run(f):
                self._check(self.lib.wn_iaf_generate_form(
                    self._h, f, _ptr(mel), B, F, _ptr(noise), ctypes.c_uint64(int(seed)), _ptr(out['wav']), _ptr(out['idx']),
                    _ptr(out['x']), _ptr(out['mean_tot']), _ptr(out['scale_tot']), _ptr(out['rand_input']), _ptr(ws),
                    ws.numel(), self._stream()))
            self._run_ranged(run, form, ws, check_range and not self.precision.startswith('f32') and form != _lib.FORM_F32 and T > 0)
        return {k: v for k, v in out.items() if k in want}

    def _window_outputs(self, B, T, want):
        """The output set of a generate call: wav always, the others where `want` names them, else None."""
        new = lambda dt=torch.float32: torch.empty((B, T), dtype=dt, device=self.device)
        return {'wav': new(), 'idx': new(torch.int32) if 'idx' in want else None, 'x': new() if 'x' in want else None,
                'mean_tot': new() if 'mean_tot' in want else None, 'scale_tot': new() if 'scale_tot' in want else None,
                'rand_input': new() if 'rand_input' in want else None}

    def _run_ranged(self, run, form, ws, read_status):
        """run(form) on workspace ws; where read_status, read the call's range word (one 4-byte read-back, which synchronises
        the stream) and re-run a call that left the fp16 range on the fp32 form."""
        run(form)
        self._last_ws = ws
        if not read_status:
            return
        rc = self.lib.wn_iaf_range_status(self._h, _ptr(ws), self._stream())
        if rc == _lib.WN_ERANGE:
            self.range_fallbacks += 1
            run(_lib.FORM_F32)      # same seed -> the same Philox draws when the noise is device-drawn
            # handled here: not to be reported again by a later check_range()
            self._check(self.lib.wn_iaf_range_reset(self._h, _ptr(ws), self._stream()))
        else:
            self._check(rc)

    # ---- the inverse of the student ----
    def iaf_encode(self, x, mel, z_init=None, max_sweeps=None, tol=0.0, check_every=8, z_max=64.0, want=('z',)):
        """The latent z with iaf_generate(mel, noise=z)['x'] == x, by fixed-point sweeps z <- (x - mean_tot(z)) / scale_tot(z)
        (wn_iaf_encode): scale_tot[t] and mean_tot[t] depend on z[<t] only, so k sweeps make the first k samples exact and T
        sweeps the whole row.  x [B,T], mel [B,F,n_mel]; starts from z_init, or from zeros.

        `check_every` sweeps are enqueued per C call; after each call front, the clamp count and the range word come back in
        ONE read-back.  The encode stops when every row's front is T (the last sweep changed no sample by more than tol;
        tol = 0: no bit) with nothing clamped to +-z_max, or at max_sweeps (default T).  All sweeps run in one arithmetic
        form: when a sweep leaves the fp16 range the encode restarts from the current iterate on the fp32 form, stays
        there, and counts into `range_fallbacks`.  The workspace is the encode's own, so the conditioning term of a shared
        deconv stack is computed once per encode.

        Returns the names in `want` out of z, mean_tot, scale_tot, log_prob (log p(x[t]), with 'log_prob_sums', float64
        [B]), plus 'sweeps' (int: sweeps until the stop condition held, or all that ran), 'front' ([B] int32), 'converged'
        ([B] bool, front == T), 'clamped' (int, of the last sweep) and 'form' (the _lib.FORM_* the sweeps ran in).
        mean_tot / scale_tot belong to the last sweep's input iterate: to z itself once it has converged.  Sweeps a C call
        has enqueued past the one where the stop condition held change nothing: z, the totals and front are that sweep's."""
        mel = self._dev(mel)
        if mel.dim() != 3 or mel.shape[2] != self.n_mel:
            raise ValueError('mel must be [batch, frames, {}], got {}'.format(self.n_mel, tuple(mel.shape)))
        B, F = int(mel.shape[0]), int(mel.shape[1])
        f32 = self.precision.startswith('f32')
        form = _lib.FORM_F32 if f32 else _lib.FORM_DEFAULT
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.wn_iaf_encode_workspace_bytes(self._h, form, B, F))
            if nbytes == 0:                # a handle or a shape the call refuses: the call itself says why
                self._check(self.lib.wn_iaf_encode(self._h, form, None, B, F, None, None, 1, 1.0, 0.0, 1, None, None, None, None,
                                                   None, 0, self._stream()))
        T = self.iaf_length(F)
        x = self._dev(x)
        if tuple(x.shape) != (B, T):
            raise ValueError('x must be [{}, {}], got {}'.format(B, T, tuple(x.shape)))
        if z_init is not None and tuple(z_init.shape) != (B, T):
            raise ValueError('z_init must be [{}, {}], got {}'.format(B, T, tuple(z_init.shape)))
        if check_every < 1:
            raise ValueError('check_every must be >= 1, got {}'.format(check_every))
        max_sweeps = T if max_sweeps is None else int(max_sweeps)
        z = torch.zeros((B, T), dtype=torch.float32, device=self.device) if z_init is None else self._dev(z_init).clone()
        new = lambda: torch.empty((B, T), dtype=torch.float32, device=self.device)
        mean_tot = new() if 'mean_tot' in want else None
        scale_tot = new() if ('scale_tot' in want or 'log_prob' in want) else None
        meta = torch.zeros(B + 4, dtype=torch.int32, device=self.device)          # front [B], then counts [4]
        sweeps, first = 0, 1
        with torch.cuda.device(self.device):
            if self._enc_ws is None or self._enc_ws.numel() < nbytes:
                self._enc_ws = None
                self._enc_ws = torch.empty(max(nbytes, 64), dtype=torch.uint8, device=self.device)
            ws = self._enc_ws
            while True:
                n = min(int(check_every), max_sweeps - sweeps)
                self._check(self.lib.wn_iaf_encode(
                    self._h, form, _ptr(mel), B, F, _ptr(x), _ptr(z), n, float(z_max), float(tol), first, _ptr(mean_tot),
                    _ptr(scale_tot), _ptr(meta), ctypes.c_void_p(meta.data_ptr() + 4 * B), _ptr(ws), ws.numel(), self._stream()))
                first = 0
                m = meta.cpu()
                front, clamped, flag, done_at = m[:B], int(m[B]), int(m[B + 1]), int(m[B + 2])
                if flag and form != _lib.FORM_F32:
                    self.range_fallbacks += 1
                    form, first = _lib.FORM_F32, 1           # z is the iterate the faulted sweep started from
                    continue
                sweeps += done_at if done_at else n
                if done_at or sweeps >= max_sweeps:
                    break
            out = {'z': z, 'mean_tot': mean_tot, 'scale_tot': scale_tot}
            if 'log_prob' in want:
                out['log_prob'], out['log_prob_sums'] = self.iaf_latent_log_prob(z, scale_tot)
        ret = {k: v for k, v in out.items() if k in want or (k == 'log_prob_sums' and 'log_prob' in want)}
        ret.update({'sweeps': sweeps, 'front': meta[:B].clone(), 'converged': meta[:B] == T, 'clamped': clamped, 'form': form})
        return ret

    def iaf_latent_log_prob(self, z, scale_tot):
        """wn_iaf_latent_log_prob: log p(x[t]) = log f(z[t]) - log scale_tot[t] of the student's (untruncated) density,
        [B,T] float32, and its row sums, [B] float64 summed in a fixed order."""
        z, scale_tot = self._dev(z), self._dev(scale_tot)
        if z.dim() != 2 or z.shape != scale_tot.shape:
            raise ValueError('z and scale_tot must be [batch, T] alike, got {} and {}'.format(tuple(z.shape), tuple(scale_tot.shape)))
        lp = torch.empty_like(z)
        sums = torch.empty(z.shape[0], dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_iaf_latent_log_prob(self._h, _ptr(z), _ptr(scale_tot), int(z.shape[0]), int(z.shape[1]),
                                                        _ptr(lp), _ptr(sums), self._stream()))
        return lp, sums

    # ---- windowed IAF generation ----
    ONE_SHOT_MAX_SAMPLES = 2000000         # twin of WN_MAX_ROW_SAMPLES (csrc/wn_internal.h): wn_iaf_generate refuses longer utterances

    def iaf_needs_windows(self, num_frames):
        """True when iaf_generate refuses num_frames for its length and iaf_generate_long has to take the call."""
        return int(num_frames) * self.frame_shift > self.ONE_SHOT_MAX_SAMPLES

    def iaf_window_geometry(self):
        """wn_iaf_window_geometry: (reach, frames_before, frames_after, period) as the library derives them;
        config.iaf_window_geometry is the Python twin."""
        r, fb, fa, p = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._check(self.lib.wn_iaf_window_geometry(self._h, ctypes.byref(r), ctypes.byref(fb), ctypes.byref(fa),
                                                    ctypes.byref(p)))
        return int(r.value), int(fb.value), int(fa.value), int(p.value)

    def iaf_generate_windows(self, mel_rows, rows, out, noise_abs=None, seed=0, form=None, form_rows=1, check_range=True,
                             ws_rows=None):
        """One wn_iaf_generate_windows call.  mel_rows [R,Fw,n_mel] on the device; rows: R tuples (b, t_origin, keep_from,
        keep_to, out_t); out: dict of [B_out,T_out] device tensors wav (required), idx, x, mean_tot, scale_tot, rand_input
        (or None) that receive the kept samples; noise_abs [B_out,T_out] or None (drawn from `seed` at absolute positions).
        check_range as in iaf_generate: a call that left the fp16 range is re-run on the fp32 form.  ws_rows: size the
        workspace for that many rows (a run of calls on one buffer)."""
        R, Fw = int(mel_rows.shape[0]), int(mel_rows.shape[1])
        if mel_rows.dim() != 3 or int(mel_rows.shape[2]) != self.n_mel or not mel_rows.is_contiguous():
            raise ValueError('mel_rows must be contiguous [rows, frames, {}], got {}'.format(self.n_mel, tuple(mel_rows.shape)))
        if len(rows) != R:
            raise ValueError('{} row descriptors for {} mel rows'.format(len(rows), R))
        wav = out['wav']
        B_out, T_out = int(wav.shape[0]), int(wav.shape[1])
        for k, v in out.items():
            if v is not None and (tuple(v.shape) != (B_out, T_out) or not v.is_contiguous()):
                raise ValueError('output {} must be contiguous [{}, {}]'.format(k, B_out, T_out))
        if noise_abs is not None and tuple(noise_abs.shape) != (B_out, T_out):
            raise ValueError('noise must be [{}, {}], got {}'.format(B_out, T_out, tuple(noise_abs.shape)))
        table = (_lib.WindowRow * R)(*[_lib.WindowRow(*[int(v) for v in r]) for r in rows])
        form = _lib.FORM_DEFAULT if form is None else form
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.wn_iaf_windows_workspace_bytes(self._h, max(R, int(ws_rows or 0)), Fw, form))

            def run(f):
                self._check(self.lib.wn_iaf_generate_windows(
                    self._h, f, int(form_rows), _ptr(mel_rows), R, Fw, table, _ptr(noise_abs), B_out, T_out,
                    ctypes.c_uint64(int(seed)), _ptr(wav), _ptr(out.get('idx')), _ptr(out.get('x')), _ptr(out.get('mean_tot')),
                    _ptr(out.get('scale_tot')), _ptr(out.get('rand_input')), _ptr(ws), ws.numel(), self._stream()))
            self._run_ranged(run, form, ws, check_range and not self.precision.startswith('f32') and form != _lib.FORM_F32)

    def iaf_generate_long(self, mel, noise=None, seed=0, want=('wav',), window_frames=None, rows_per_call=8, crop='centre',
                          check_range=True, form=None, out=None):
        """iaf_generate for any number of frames: the utterance is planned as windows of one frame count
        (config.iaf_plan_windows), each recomputing the `reach` samples of causal context in front of what it keeps, and
        the windows run as batches of rows_per_call rows on one workspace, writing into one output set.  Same keys and
        shapes as iaf_generate.  A plan of ONE row (F <= window_frames; default 384 frames for the shipped configs) returns
        iaf_generate's bits; otherwise x, mean_tot and scale_tot agree with it to the accuracy two calls of different
        length agree, and the device noise is the one-shot's noise bit for bit.
        crop='left' crops the conditioning on the right only (sample t reads upsampled column t) -- what a stream produces;
        it coincides with the one-shot's centred crop whenever F % period == 0.  form: a _lib.FORM_* (default: the engine's).
        out: preallocated [B,T] device tensors under iaf_generate_windows' names ('wav' at least), to be written instead of
        new ones."""
        mel = self._dev(mel)
        if mel.dim() != 3 or mel.shape[2] != self.n_mel:
            raise ValueError('mel must be [batch, frames, {}], got {}'.format(self.n_mel, tuple(mel.shape)))
        if int(rows_per_call) < 1:
            raise ValueError('rows_per_call must be >= 1')
        B, F = int(mel.shape[0]), int(mel.shape[1])
        T = self.iaf_length(F)
        noise = self._dev(noise)
        if noise is not None and tuple(noise.shape) != (B, T):
            raise ValueError('noise must be [{}, {}], got {}'.format(B, T, tuple(noise.shape)))
        out = dict(out) if out is not None else self._window_outputs(B, T, want)
        if T > 0:
            Fw, plan = cfg.iaf_plan_windows(self.hp, F, window_frames, crop)
            rows = [(b, f0) + (to, kf, kt, ot) for (f0, to, kf, kt, ot) in plan for b in range(B)]
            # a single-row plan is the one-shot: its launch form is chosen for the whole batch, as iaf_generate chooses it
            form_rows = B if len(plan) == 1 else 1
            n = min(int(rows_per_call), len(rows))
            for i in range(0, len(rows), n):
                part = rows[i:i + n]
                mel_rows = torch.stack([mel[b, f0:f0 + Fw] for b, f0 in (r[:2] for r in part)])
                self.iaf_generate_windows(mel_rows, [(r[0],) + r[2:] for r in part], out, noise, seed, form, form_rows,
                                          check_range, ws_rows=n)
        return {k: v for k, v in out.items() if k in want}

    def iaf_stream(self, batch=1, seed=0, window_frames=None, want=('wav',)):
        """A streaming generator: see IafStream."""
        return IafStream(self, batch, seed, window_frames, want)

    def check_range(self):
        """Raise if any iaf_generate(check_range=False) call since the last check left the fp16 range (the outputs of
        such a call are NaN); synchronises the stream once."""
        if self._last_ws is None or self.precision.startswith('f32'):
            return
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_iaf_range_status_since_reset(self._h, _ptr(self._last_ws), self._stream()))

    def clip_quant(self, x):
        x = self._dev(x)
        wav = torch.empty_like(x)
        idx = torch.empty(x.shape, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_clip_quant(self._h, _ptr(x), x.numel(), _ptr(wav), _ptr(idx), self._stream()))
        return wav, idx

    def _deconv_scope(self, scope):
        if scope is not None:
            return scope
        return '' if self.kind == 'teacher' else \
            ('iaf_share' if (getattr(self.hp, 'use_share_deconv', False) or
                             getattr(self.hp, 'use_teacher_deconv', False)) else 'iaf_1')

    def deconv_forms(self, batch, num_frames, scope=None, split_out=False, precision=None):
        """The kernels the upsampler stack `scope` runs for (batch, num_frames), one string per layer ('front', 'pg',
        'hs<4> il', 'h<false> g4<10>', 'fa g4<0>', 'mfma il' ...: wn_deconv_forms).  split_out: G4 words out, as the generate,
        teacher and training calls ask for, instead of deconv()'s fp32 rows; precision: None = the engine's, else 'f16x3' or
        'f32' for the arithmetic of one call.  Launches nothing."""
        prec = -1 if precision is None else cfg.PRECISIONS[precision][0]
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.wn_deconv_forms(self._h, self._deconv_scope(scope).encode(), int(batch), int(num_frames),
                                             int(bool(split_out)), prec, buf, len(buf)))
        return buf.value.decode().split(', ')

    def deconv(self, mel, scope=None):
        """Wavenet.deconv_stack: mel [B,F,n_mel] -> [B, F*frame_shift, deconv_width]."""
        mel = self._dev(mel)
        B, F = int(mel.shape[0]), int(mel.shape[1])
        scope = self._deconv_scope(scope)
        enc = torch.empty((B, F * self.frame_shift, self.hp.deconv_width), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.lib.wn_workspace_bytes(self._h, B, F))
            self._check(self.lib.wn_deconv(self._h, scope.encode(), _ptr(mel), B, F, _ptr(enc), _ptr(ws),
                                           ws.numel(), self._stream()))
        return enc

    # ---- teacher, whole sequence at once ----
    def teacher_forward(self, wav, mel):
        """Wavenet.feed_forward (wavenet.py:180-291): wav [B,T] raw audio, mel [B,F,n_mel] ->
        out_params [B,T,out_width].  T <= F*frame_shift, multiple of the largest dilation."""
        wav, mel = self._dev(wav), self._dev(mel)
        if wav.dim() != 2 or mel.dim() != 3 or wav.shape[0] != mel.shape[0]:
            raise ValueError('teacher_forward: wav must be [B,T] and mel [B,F,n_mel] with equal B')
        if int(mel.shape[2]) != self.n_mel:
            raise ValueError('teacher_forward: mel has {} channels, the model expects {}'.format(
                int(mel.shape[2]), self.n_mel))
        B, T, F = int(wav.shape[0]), int(wav.shape[1]), int(mel.shape[1])
        out = torch.empty((B, T, cfg.teacher_out_width(self.hp)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.lib.wn_teacher_workspace_bytes(self._h, B, F, T)
            ws = self._workspace(max(int(nb), 256))
            self._check(self.lib.wn_teacher_forward(self._h, _ptr(wav), _ptr(mel), B, F, T, _ptr(out), _ptr(ws),
                                                    ws.numel(), self._stream()))
        return out

    def _log_prob_args(self, what, out_params, wav):
        out_params, wav = self._dev(out_params), self._dev(wav)
        ow = cfg.teacher_out_width(self.hp) if self.kind == 'teacher' else None    # a student handle: the library refuses
        if wav.dim() != 2 or out_params.dim() != 3 or tuple(out_params.shape[:2]) != tuple(wav.shape) or \
                (ow is not None and int(out_params.shape[2]) != ow):
            raise ValueError('{}: out_params must be [B,T,{}] and wav [B,T]'.format(what, ow))
        return out_params, wav

    def teacher_log_prob(self, out_params, wav):
        """Per-sample log-likelihood of wav [B,T] under out_params [B,T,out_width] (loss_func.py:22-63,104-119,128-133 on the
        targets of Wavenet.encode_signal, wavenet.py:157-178) -> [B,T]; Wavenet.calculate_loss's 'loss' is minus its mean."""
        out_params, wav = self._log_prob_args('teacher_log_prob', out_params, wav)
        lp = torch.empty(tuple(wav.shape), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_teacher_log_prob(self._h, _ptr(out_params), _ptr(wav), int(wav.shape[0]), int(wav.shape[1]),
                                                     _ptr(lp), self._stream()))
        return lp

    def teacher_log_prob_grad(self, out_params, wav, d_log_prob, want_wav=True):
        """Gradient of teacher_log_prob: d_log_prob [B,T] -> (d out_params [B,T,out_width], d wav [B,T] through
        the target, or None without want_wav).  d wav is zero for mu-law and ce teachers (the target is quantised audio)."""
        out_params, wav = self._log_prob_args('teacher_log_prob_grad', out_params, wav)
        g = self._dev(d_log_prob)
        if tuple(g.shape) != tuple(wav.shape):
            raise ValueError('teacher_log_prob_grad: d_log_prob must be [B,T] = {}, got {}'.format(tuple(wav.shape), tuple(g.shape)))
        d_out = torch.empty_like(out_params)
        d_wav = torch.empty_like(wav) if want_wav else None
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_teacher_log_prob_grad(self._h, _ptr(out_params), _ptr(wav), int(wav.shape[0]),
                                                          int(wav.shape[1]), _ptr(g), _ptr(d_out), _ptr(d_wav), self._stream()))
        return d_out, d_wav

    # ---- distillation losses (teacher handle; ParallelWavenet.kl_loss_logistic / kl_loss_gauss) ----
    def _distill_args(self, what, out_params, mean_tot, scale_tot):
        out_params, mean_tot, scale_tot = self._dev(out_params), self._dev(mean_tot), self._dev(scale_tot)
        if mean_tot.dim() != 2 or out_params.dim() != 3 or tuple(scale_tot.shape) != tuple(mean_tot.shape) or \
                tuple(out_params.shape[:2]) != tuple(mean_tot.shape):
            raise ValueError('{}: out_params must be [B,T,out_width], mean_tot and scale_tot [B,T]'.format(what))
        return out_params, mean_tot, scale_tot

    def distill_mol_xent(self, out_params, mean_tot, scale_tot, num_samples, noise=None, seed=0, want_noise=False):
        """The Monte-Carlo cross entropy of kl_loss_logistic (parallel_wavenet.py:361-402) under this MoL teacher:
        out_params [B,T,3 mol_mix] (teacher_forward of the student's x), the student's mean_tot / scale_tot [B,T].
        noise: [B,num_samples,T] injected logistic draws, or None (Philox on the device from `seed`).
        Returns {'H_bl': [B,T] float32, 'sums': [2] float64 (sum of H_bl, sum of log scale_tot)} and 'noise' [B,S,T]
        (the draws used) when want_noise."""
        out_params, mean_tot, scale_tot = self._distill_args('distill_mol_xent', out_params, mean_tot, scale_tot)
        B, T, S = int(mean_tot.shape[0]), int(mean_tot.shape[1]), int(num_samples)
        noise = self._dev(noise)
        if noise is not None and tuple(noise.shape) != (B, S, T):
            raise ValueError('distill_mol_xent: noise must be [B, num_samples, T] = [{}, {}, {}]'.format(B, S, T))
        h_bl = torch.empty((B, T), dtype=torch.float32, device=self.device)
        sums = torch.empty(2, dtype=torch.float64, device=self.device)
        nout = torch.empty((B, S, T), dtype=torch.float32, device=self.device) if want_noise and S > 0 else None
        with torch.cuda.device(self.device):
            ws = self._workspace(max(int(self.lib.wn_distill_workspace_bytes(self._h, B, T)), 256))
            self._check(self.lib.wn_distill_mol_xent(self._h, _ptr(out_params), int(out_params.shape[2]), _ptr(mean_tot),
                                                     _ptr(scale_tot), B, T, S, _ptr(noise), ctypes.c_uint64(seed & (2 ** 64 - 1)),
                                                     _ptr(h_bl), _ptr(nout), _ptr(sums), _ptr(ws), ws.numel(), self._stream()))
        out = {'H_bl': h_bl, 'sums': sums}
        if want_noise:
            out['noise'] = nout
        return out

    def distill_gauss_kl(self, out_params, mean_tot, scale_tot):
        """kl_loss_gauss (parallel_wavenet.py:404-429) under this Gauss teacher: out_params [B,T,2], the student's
        mean_tot / scale_tot [B,T].  Returns {'kl_bl': [B,T] float32, 'sums': [2] float64 (sum of kl_bl, sum of the
        squared log-scale differences)}."""
        out_params, mean_tot, scale_tot = self._distill_args('distill_gauss_kl', out_params, mean_tot, scale_tot)
        B, T = int(mean_tot.shape[0]), int(mean_tot.shape[1])
        kl_bl = torch.empty((B, T), dtype=torch.float32, device=self.device)
        sums = torch.empty(2, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(max(int(self.lib.wn_distill_workspace_bytes(self._h, B, T)), 256))
            self._check(self.lib.wn_distill_gauss_kl(self._h, _ptr(out_params), int(out_params.shape[2]), _ptr(mean_tot),
                                                     _ptr(scale_tot), B, T, _ptr(kl_bl), _ptr(sums), _ptr(ws), ws.numel(),
                                                     self._stream()))
        return {'kl_bl': kl_bl, 'sums': sums}

    # ---- gradients of the distillation losses (autograd Functions in distill_autograd.py) ----
    # Every call below takes its workspace from torch's allocator per call (no shared buffer): they also run on the autograd
    # engine's device thread, on the stream torch makes current there.
    def teacher_tape_bytes(self, B, T):
        return int(self.lib.wn_teacher_tape_bytes(self._h, int(B), int(T)))

    def teacher_forward_tape(self, wav, mel):
        """teacher_forward (bit-identical out_params) that also returns the tape the input VJP reads: a uint8 device tensor
        of teacher_tape_bytes(B, T) bytes."""
        wav, mel = self._dev(wav), self._dev(mel)
        if wav.dim() != 2 or mel.dim() != 3 or wav.shape[0] != mel.shape[0]:
            raise ValueError('teacher_forward_tape: wav must be [B,T] and mel [B,F,n_mel] with equal B')
        if int(mel.shape[2]) != self.n_mel:
            raise ValueError('teacher_forward_tape: mel has {} channels, the model expects {}'.format(
                int(mel.shape[2]), self.n_mel))
        B, T, F = int(wav.shape[0]), int(wav.shape[1]), int(mel.shape[1])
        out = torch.empty((B, T, cfg.teacher_out_width(self.hp)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            tape = torch.empty(max(self.teacher_tape_bytes(B, T), 256), dtype=torch.uint8, device=self.device)
            ws = torch.empty(max(int(self.lib.wn_teacher_workspace_bytes(self._h, B, F, T)), 256), dtype=torch.uint8,
                             device=self.device)
            self._check(self.lib.wn_teacher_forward_tape(self._h, _ptr(wav), _ptr(mel), B, F, T, _ptr(out), _ptr(tape),
                                                         tape.numel(), _ptr(ws), ws.numel(), self._stream()))
        return out, tape

    def teacher_backward_input(self, tape, d_out_params):
        """Input VJP of the teacher: d_out_params [B,T,out_width] -> d wav [B,T] on a tape of teacher_forward_tape."""
        g = self._dev(d_out_params)
        if g.dim() != 3 or (self.kind == 'teacher' and int(g.shape[2]) != cfg.teacher_out_width(self.hp)):
            raise ValueError('teacher_backward_input: d_out_params must be [B,T,{}]'.format(cfg.teacher_out_width(self.hp)))
        B, T = int(g.shape[0]), int(g.shape[1])
        dwav = torch.empty((B, T), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = torch.empty(max(int(self.lib.wn_teacher_backward_workspace_bytes(self._h, B, T)), 256), dtype=torch.uint8,
                             device=self.device)
            self._check(self.lib.wn_teacher_backward_input(self._h, _ptr(tape), tape.numel(), _ptr(g), B, T, _ptr(dwav),
                                                           _ptr(ws), ws.numel(), self._stream()))
        return dwav

    # ---- gradient tables of the weight-gradient calls: one flat float32 buffer, one entry per TF variable ----
    def _grad_table(self, key, count, info, *prefix_args):
        """[(tf variable name, float offset, TF shape)] from a wn_*_grad_count / wn_*_grad_info pair (prefix_args: what the
        pair takes between the handle and the index).  The layout of a finalized handle is fixed, so its table is walked
        once and kept under `key` for the handle's forks too; the caller gets a list of its own.  Nothing is kept of an
        engine that is not finalized or of a model the calls refuse."""
        tables = self._shared['grad_tables']
        if key in tables:
            return list(tables[key])
        out = []
        name = ctypes.create_string_buffer(160)
        off, nd, shape = ctypes.c_int64(0), ctypes.c_int(0), (ctypes.c_int64 * 4)()
        for i in range(int(count(self._h, *prefix_args))):
            self._check(info(self._h, *prefix_args, i, name, 160, ctypes.byref(off), shape, ctypes.byref(nd)))
            out.append((name.value.decode(), int(off.value), tuple(int(shape[k]) for k in range(nd.value))))
        if self._finalized and out:
            tables[key] = tuple(out)
        return out

    @staticmethod
    def _grad_views(flat, table):
        """{tf name: view of the flat buffer in the TF shape}"""
        return {name: flat[off:off + int(np.prod(shape))].view(shape) for name, off, shape in table}

    # ---- weight gradients of the teacher ----
    def teacher_train_tape_bytes(self, B, F, T):
        return int(self.lib.wn_teacher_train_tape_bytes(self._h, int(B), int(F), int(T)))

    def teacher_grad_table(self):
        """[(tf variable name, float offset, TF shape)] of the flat gradient buffer, in the library's fixed order."""
        return self._grad_table(('teacher', ''), self.lib.wn_teacher_grad_count, self.lib.wn_teacher_grad_info)

    DROPOUT_MODES = {'dropout_inputs': 1, 'dropout_all': 2}        # WN_DROPOUT_INPUTS, WN_DROPOUT_ALL

    def teacher_dropout_keep(self, seed, site, B, C, T, rate):
        """The keep bits of dropout site `site` as the device evaluates them: bool [B,T,C], written by a kernel
        that only calls the hash the training passes call.  train.dropout_keep is its numpy twin."""
        keep = torch.empty((int(B), int(T), int(C)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_teacher_dropout_keep(ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(site), int(B), int(C),
                                                         int(T), float(rate), _ptr(keep), self._stream()))
        return keep.bool()

    def teacher_forward_train_tape(self, wav, mel, dropout=None):
        """teacher_forward (bit-identical out_params) that also returns the TRAINING tape teacher_backward_weights reads: the
        tape of teacher_forward_tape plus every layer's input, the conditioning and the scaled audio.  teacher_backward_input
        accepts it too.  The engine remembers the tape's frame count by its address.
        dropout = (mode, seed, rate), mode 'dropout_inputs' or 'dropout_all' (or WN_DROPOUT_INPUTS / WN_DROPOUT_ALL): the
        forward of train_wavenet.py with tf.layers.dropout(training=True) under the counter-hash mask of DESIGN.md 17;
        out_params are those of the dropped forward and the reverse calls apply the same masks.  None: no dropout."""
        if dropout is not None:
            mode, seed, rate = dropout
            mode = self.DROPOUT_MODES.get(mode, 0) if isinstance(mode, str) else int(mode)    # unknown: the library refuses
            seed = ctypes.c_uint64(int(seed) & (2 ** 64 - 1))
        wav, mel = self._dev(wav), self._dev(mel)
        if wav.dim() != 2 or mel.dim() != 3 or wav.shape[0] != mel.shape[0]:
            raise ValueError('teacher_forward_train_tape: wav must be [B,T] and mel [B,F,n_mel] with equal B')
        if int(mel.shape[2]) != self.n_mel:
            raise ValueError('teacher_forward_train_tape: mel has {} channels, the model expects {}'.format(
                int(mel.shape[2]), self.n_mel))
        B, T, F = int(wav.shape[0]), int(wav.shape[1]), int(mel.shape[1])
        out = torch.empty((B, T, cfg.teacher_out_width(self.hp)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = self.teacher_train_tape_bytes(B, F, T) if dropout is None else \
                int(self.lib.wn_teacher_train_tape_dropout_bytes(self._h, B, F, T, mode))
            tape = torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)
            ws = torch.empty(max(int(self.lib.wn_teacher_workspace_bytes(self._h, B, F, T)), 256), dtype=torch.uint8,
                             device=self.device)
            if dropout is None:
                self._check(self.lib.wn_teacher_forward_train_tape(self._h, _ptr(wav), _ptr(mel), B, F, T, _ptr(out), _ptr(tape),
                                                                   tape.numel(), _ptr(ws), ws.numel(), self._stream()))
            else:
                self._check(self.lib.wn_teacher_forward_train_tape_dropout(
                    self._h, _ptr(wav), _ptr(mel), B, F, T, _ptr(out), _ptr(tape), tape.numel(), _ptr(ws), ws.numel(),
                    self._stream(), mode, seed, float(rate)))
        # the library identifies a tape by its address (a copy is refused), so the frame count is kept by address too
        if len(self._train_frames) >= 256:
            self._train_frames.clear()
        self._train_frames[tape.data_ptr()] = F
        return out, tape

    def teacher_backward_weights(self, tape, d_out_params, n_frames=None, want_encoding=False, want_wav=False):
        """One reverse pass on a tape of teacher_forward_train_tape: d_out_params [B,T,out_width] ->
        {'grads': {tf name: device tensor in the TF shape} (views into 'flat_grads'), 'flat_grads': [n] float32,
        'd_encoding': [B, F frame_shift, deconv_width] or None, 'd_wav': [B,T] (teacher_backward_input's bits) or None}."""
        g = self._dev(d_out_params)
        if g.dim() != 3 or (self.kind == 'teacher' and int(g.shape[2]) != cfg.teacher_out_width(self.hp)):
            raise ValueError('teacher_backward_weights: d_out_params must be [B,T,{}]'.format(cfg.teacher_out_width(self.hp)))
        F = int(n_frames if n_frames is not None else self._train_frames.get(tape.data_ptr(), 0))
        if F < 1:
            raise ValueError('teacher_backward_weights: pass n_frames for a tape this engine object did not write')
        B, T = int(g.shape[0]), int(g.shape[1])
        with torch.cuda.device(self.device):
            n = int(self.lib.wn_teacher_grad_floats(self._h))
            flat = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
            denc = torch.empty((B, F * self.frame_shift, int(self.hp.deconv_width)), dtype=torch.float32, device=self.device) \
                if want_encoding else None
            dwav = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_wav else None
            ws = torch.empty(max(int(self.lib.wn_teacher_backward_weights_workspace_bytes(self._h, B, F, T)), 256),
                             dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_teacher_backward_weights(self._h, _ptr(tape), tape.numel(), _ptr(g), B, F, T, _ptr(flat), n,
                                                             _ptr(denc), _ptr(dwav), _ptr(ws), ws.numel(), self._stream()))
            grads = self._grad_views(flat, self.teacher_grad_table())
        return {'grads': grads, 'flat_grads': flat[:n], 'd_encoding': denc, 'd_wav': dwav}

    # ---- weight gradients of the student ----
    def iaf_grad_table(self):
        """[(tf variable name, float offset, TF shape)] of iaf_backward_weights' flat gradient buffer: every variable of every
        flow in the order weights.expected_variables lists them (the upsampler's are deconv_backward's).  Empty for a
        model the training calls refuse."""
        return self._grad_table(('iaf', ''), self.lib.wn_iaf_grad_count, self.lib.wn_iaf_grad_info)

    def iaf_train_tape_bytes(self, B, F):
        return int(self.lib.wn_iaf_train_tape_bytes(self._h, int(B), int(F), self.iaf_length(F)))

    def iaf_forward_train_tape(self, mel, noise=None, seed=0):
        """ParallelWavenet.feed_forward for training: mel [B,F,n_mel] -> ({'x', 'mean_tot', 'scale_tot', 'rand_input'}, tape),
        each tensor [B,T] on the device, the tape a uint8 device tensor iaf_backward_weights reads (identified by its
        address).  noise [B,T] injects the draw; None draws it with iaf_generate's generator from `seed`."""
        mel = self._dev(mel)
        if mel.dim() != 3 or mel.shape[2] != self.n_mel:
            raise ValueError('mel must be [batch, frames, {}], got {}'.format(self.n_mel, tuple(mel.shape)))
        B, F = int(mel.shape[0]), int(mel.shape[1])
        T = self.iaf_length(F)
        if noise is None:
            noise = self.iaf_generate(mel, seed=seed, want=('rand_input',), check_range=False)['rand_input']
        noise = self._dev(noise)
        if tuple(noise.shape) != (B, T):
            raise ValueError('noise must be [{}, {}], got {}'.format(B, T, tuple(noise.shape)))
        new = lambda: torch.empty((B, T), dtype=torch.float32, device=self.device)
        x, mt, st = new(), new(), new()
        with torch.cuda.device(self.device):
            tape = torch.empty(max(int(self.lib.wn_iaf_train_tape_bytes(self._h, B, F, T)), 256), dtype=torch.uint8,
                               device=self.device)
            ws = torch.empty(max(int(self.lib.wn_iaf_train_workspace_bytes(self._h, B, F, T)), 256), dtype=torch.uint8,
                             device=self.device)
            self._check(self.lib.wn_iaf_forward_train_tape(self._h, _ptr(noise), _ptr(mel), B, F, T, _ptr(x), _ptr(mt),
                                                           _ptr(st), _ptr(tape), tape.numel(), _ptr(ws), ws.numel(),
                                                           self._stream()))
        if len(self._train_frames) >= 256:
            self._train_frames.clear()
        self._train_frames[tape.data_ptr()] = F
        return {'x': x, 'mean_tot': mt, 'scale_tot': st, 'rand_input': noise}, tape

    def iaf_n_stacks(self):
        """deconv stacks of the student: 1 when shared or teacher-owned, else one per flow"""
        share = getattr(self.hp, 'use_share_deconv', False) or getattr(self.hp, 'use_teacher_deconv', False)
        return 1 if share else max(1, len(getattr(self.hp, 'num_iaf_layers', ())))

    def iaf_backward_weights(self, tape, d_x, d_mean_tot, d_scale_tot, want_encoding=True, n_frames=None):
        """One reverse pass on a tape of iaf_forward_train_tape.  d_x, d_mean_tot, d_scale_tot [B,T]: the cotangents of the
        three returned tensors as independent outputs (x's dependence on the other two is added by the call) ->
        {'grads': {tf name: device tensor in the TF shape} (views into 'flat_grads'), 'flat_grads': [n] float32,
        'd_encoding': [n_stacks, B, F frame_shift, deconv_width] or None}."""
        g = [self._dev(v) for v in (d_x, d_mean_tot, d_scale_tot)]
        if g[0].dim() != 2 or any(tuple(v.shape) != tuple(g[0].shape) for v in g):
            raise ValueError('iaf_backward_weights: d_x, d_mean_tot and d_scale_tot must be [B,T]')
        F = int(n_frames if n_frames is not None else self._train_frames.get(tape.data_ptr(), 0))
        if F < 1:
            raise ValueError('iaf_backward_weights: pass n_frames for a tape this engine object did not write')
        B, T = int(g[0].shape[0]), int(g[0].shape[1])
        with torch.cuda.device(self.device):
            n = int(self.lib.wn_iaf_grad_floats(self._h))
            flat = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
            denc = torch.empty((self.iaf_n_stacks(), B, F * self.frame_shift, int(self.hp.deconv_width)), dtype=torch.float32,
                               device=self.device) if want_encoding else None
            ws = torch.empty(max(int(self.lib.wn_iaf_backward_weights_workspace_bytes(self._h, B, F, T)), 256),
                             dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_iaf_backward_weights(self._h, _ptr(tape), tape.numel(), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                                         B, F, T, _ptr(flat), n, _ptr(denc), _ptr(ws), ws.numel(),
                                                         self._stream()))
            grads = self._grad_views(flat, self.iaf_grad_table())
        return {'grads': grads, 'flat_grads': flat[:n], 'd_encoding': denc}

    def iaf_backward_input(self, tape, d_x, d_mean_tot, d_scale_tot, want_encoding=True, n_frames=None):
        """iaf_backward_weights' reverse pass on the same tape without the weight products: the cotangents of
        the three returned tensors -> {'d_noise': [B,T], the gradient of the draw iaf_forward_train_tape was given,
        'd_encoding': [n_stacks, B, F frame_shift, deconv_width] (iaf_backward_weights' bits) or None}."""
        g = [self._dev(v) for v in (d_x, d_mean_tot, d_scale_tot)]
        if g[0].dim() != 2 or any(tuple(v.shape) != tuple(g[0].shape) for v in g):
            raise ValueError('iaf_backward_input: d_x, d_mean_tot and d_scale_tot must be [B,T]')
        F = int(n_frames if n_frames is not None else self._train_frames.get(tape.data_ptr(), 0))
        if F < 1:
            raise ValueError('iaf_backward_input: pass n_frames for a tape this engine object did not write')
        B, T = int(g[0].shape[0]), int(g[0].shape[1])
        with torch.cuda.device(self.device):
            dn = torch.empty((B, T), dtype=torch.float32, device=self.device)
            denc = torch.empty((self.iaf_n_stacks(), B, F * self.frame_shift, int(self.hp.deconv_width)), dtype=torch.float32,
                               device=self.device) if want_encoding else None
            ws = torch.empty(max(int(self.lib.wn_iaf_backward_input_workspace_bytes(self._h, B, F, T)), 256),
                             dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_iaf_backward_input(self._h, _ptr(tape), tape.numel(), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                                       B, F, T, _ptr(dn), _ptr(denc), _ptr(ws), ws.numel(), self._stream()))
        return {'d_noise': dn, 'd_encoding': denc}

    # ---- the gradient of the student's log-likelihood ----
    ADJOINT_TOL = 1e-5          # the default tolerance of iaf_adjoint: DESIGN.md 27.3 has the measurements behind it

    def iaf_latent_log_prob_grad(self, z, scale_tot, d_log_prob=None):
        """wn_iaf_latent_log_prob_grad, iaf_latent_log_prob's counterpart: for a cotangent d_log_prob [B,T] of log p (None:
        the constant -1 / (B T) of -mean log p) -> (g_z, d_scale_tot), [B,T] float32: d_log_prob (log f)'(z) and
        -d_log_prob / scale_tot."""
        z, scale_tot, d_log_prob = self._dev(z), self._dev(scale_tot), self._dev(d_log_prob)
        if z.dim() != 2 or z.shape != scale_tot.shape or (d_log_prob is not None and d_log_prob.shape != z.shape):
            raise ValueError('z, scale_tot and d_log_prob must be [batch, T] alike, got {}'.format(
                [tuple(v.shape) for v in (z, scale_tot, d_log_prob) if v is not None]))
        g_z, d_s = torch.empty_like(z), torch.empty_like(z)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_iaf_latent_log_prob_grad(self._h, _ptr(z), _ptr(scale_tot), int(z.shape[0]), int(z.shape[1]),
                                                             _ptr(d_log_prob), _ptr(g_z), _ptr(d_s), self._stream()))
        return g_z, d_s

    def iaf_adjoint(self, tape, g_z, d_scale_tot, d_mean_tot=None, lam_init=None, max_sweeps=None, tol=ADJOINT_TOL, check_every=8,
                    n_frames=None):
        """The adjoint of the inverse (wn_iaf_adjoint): on a tape of iaf_forward_train_tape at noise = z, solve
        A^T lam = g_z + (d scale_tot / d z)^T d_scale_tot (+ the same of d_mean_tot), A = d x / d z, by Jacobi sweeps
        lam <- lam + (g_z + r) / scale_tot with r = iaf_backward_input(tape, -lam, d_mean_tot, d_scale_tot)['d_noise'].  A^T is
        upper triangular: k sweeps make the last k samples of a row exact, T sweeps the row.  Starts from lam_init, or zeros.

        `check_every` sweeps are enqueued per C call, then the residuals and counts come back in ONE read-back.  The solve
        stops after the first sweep in which every row had max |lam' - lam| <= tol max |lam'|, or at max_sweeps (default T);
        sweeps a C call has enqueued past that one change nothing, so the result does not depend on check_every.
        Returns {'lam' [B,T], 'sweeps' (int), 'converged' ([B] bool), 'resid' ([B,2] float32: max |lam' - lam|, max |lam'| of
        the last sweep), 'replaced' (int: non-finite values the last sweep replaced by 0)}."""
        g_z, d_scale_tot, d_mean_tot = self._dev(g_z), self._dev(d_scale_tot), self._dev(d_mean_tot)
        if g_z.dim() != 2 or any(v is not None and tuple(v.shape) != tuple(g_z.shape) for v in (d_scale_tot, d_mean_tot, lam_init)):
            raise ValueError('iaf_adjoint: g_z, d_scale_tot, d_mean_tot and lam_init must be [B,T] alike')
        F = int(n_frames if n_frames is not None else self._train_frames.get(tape.data_ptr(), 0))
        if F < 1:
            raise ValueError('iaf_adjoint: pass n_frames for a tape this engine object did not write')
        if check_every < 1:
            raise ValueError('check_every must be >= 1, got {}'.format(check_every))
        B, T = int(g_z.shape[0]), int(g_z.shape[1])
        max_sweeps = T if max_sweeps is None else int(max_sweeps)
        lam = torch.zeros((B, T), dtype=torch.float32, device=self.device) if lam_init is None else self._dev(lam_init).clone()
        meta = torch.zeros(2 * B + 4, dtype=torch.int32, device=self.device)          # resid [B][2] (float32), then counts [4]
        sweeps, replaced = 0, 0
        with torch.cuda.device(self.device):
            ws = torch.empty(max(int(self.lib.wn_iaf_adjoint_workspace_bytes(self._h, B, F, T)), 256), dtype=torch.uint8,
                             device=self.device)
            while True:
                n = min(int(check_every), max_sweeps - sweeps)
                self._check(self.lib.wn_iaf_adjoint(
                    self._h, _ptr(tape), tape.numel(), _ptr(g_z), _ptr(d_mean_tot), _ptr(d_scale_tot), B, F, T, _ptr(lam), n,
                    float(tol), _ptr(meta), ctypes.c_void_p(meta.data_ptr() + 8 * B), _ptr(ws), ws.numel(), self._stream()))
                m = meta.cpu()
                replaced, done_at = int(m[2 * B]), int(m[2 * B + 2])
                sweeps += done_at if done_at else n
                if done_at or sweeps >= max_sweeps:
                    break
        resid = meta[:2 * B].view(torch.float32).view(B, 2).clone()
        return {'lam': lam, 'sweeps': sweeps, 'converged': resid[:, 0] <= torch.tensor(tol, dtype=torch.float32) * resid[:, 1],
                'resid': resid, 'replaced': replaced}

    # ---- reverse pass of the upsampler ----
    def deconv_grad_table(self, scope=''):
        """[(tf variable name, float offset, TF shape)] of deconv_backward's flat gradient buffer: per layer
        '<scope/>trans_conv_j/kernel' [1,K,Cout,Cin], then '<scope/>trans_conv_j/bias' [Cout].  Empty for a stack the call
        refuses."""
        return self._grad_table(('deconv', scope), self.lib.wn_deconv_grad_count, self.lib.wn_deconv_grad_info, scope.encode())

    def deconv_backward(self, mel, d_encoding, scope=''):
        """VJP of deconv(mel, scope) with respect to the stack's variables: mel [B,F,n_mel] and a cotangent d_encoding
        [B, F frame_shift, deconv_width] -> {'grads': {tf name: device tensor in the TF shape} (views into 'flat_grads'),
        'flat_grads': [n] float32}.  Reruns the stack's forward; no tape."""
        mel, g = self._dev(mel), self._dev(d_encoding)
        if mel.dim() != 3 or int(mel.shape[2]) != self.n_mel:
            raise ValueError('deconv_backward: mel must be [B,F,{}]'.format(self.n_mel))
        B, F = int(mel.shape[0]), int(mel.shape[1])
        want = (B, F * self.frame_shift, int(self.hp.deconv_width))
        if tuple(g.shape) != want:
            raise ValueError('deconv_backward: d_encoding must be [B, F frame_shift, deconv_width] = {}, got {}'.format(
                list(want), list(g.shape)))
        sc = scope.encode()
        with torch.cuda.device(self.device):
            n = int(self.lib.wn_deconv_grad_floats(self._h, sc))
            flat = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
            ws = torch.empty(max(int(self.lib.wn_deconv_backward_workspace_bytes(self._h, sc, B, F)), 256), dtype=torch.uint8,
                             device=self.device)
            self._check(self.lib.wn_deconv_backward(self._h, sc, _ptr(mel), _ptr(g), B, F, _ptr(flat), n, _ptr(ws), ws.numel(),
                                                    self._stream()))
            grads = self._grad_views(flat, self.deconv_grad_table(scope))
        return {'grads': grads, 'flat_grads': flat[:n]}

    def deconv_backward_input(self, mel, d_encoding, scope=''):
        """VJP of deconv(mel, scope) with respect to mel: mel [B,F,n_mel] and a cotangent d_encoding
        [B, F frame_shift, deconv_width] -> d_mel [B,F,n_mel].  Reruns the stack's forward like deconv_backward; no tape, no
        weight gradients."""
        mel, g = self._dev(mel), self._dev(d_encoding)
        if mel.dim() != 3 or int(mel.shape[2]) != self.n_mel:
            raise ValueError('deconv_backward_input: mel must be [B,F,{}]'.format(self.n_mel))
        B, F = int(mel.shape[0]), int(mel.shape[1])
        want = (B, F * self.frame_shift, int(self.hp.deconv_width))
        if tuple(g.shape) != want:
            raise ValueError('deconv_backward_input: d_encoding must be [B, F frame_shift, deconv_width] = {}, got {}'.format(
                list(want), list(g.shape)))
        sc = scope.encode()
        with torch.cuda.device(self.device):
            d_mel = torch.empty((B, F, self.n_mel), dtype=torch.float32, device=self.device)
            ws = torch.empty(max(int(self.lib.wn_deconv_backward_input_workspace_bytes(self._h, sc, B, F)), 256),
                             dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_deconv_backward_input(self._h, sc, _ptr(mel), _ptr(g), B, F, _ptr(d_mel), _ptr(ws),
                                                          ws.numel(), self._stream()))
        return d_mel

    # ---- training step on the device (the trainer is train.TeacherTrainer) ----
    def teacher_set_weights(self, params, up_params=None):
        """Re-pack this finalized teacher's weights in place from flat float32 device buffers: `params` in the layout of
        teacher_grad_table(), `up_params` in that of deconv_grad_table('') or None (the upsampler keeps its weights).  The
        handle then holds what load_weights of the same values would have built.  Synchronises the current stream once (the
        scales' maxima are read back); tapes written before the call are refused afterwards.  A switch: RuntimeError
        (WN_ESTATE) while another thread's work call is inside the library."""
        _flat_f32('teacher_set_weights', 'params', params)
        if up_params is not None:
            _flat_f32('teacher_set_weights', 'up_params', up_params)
        with torch.cuda.device(self.device):
            nb = int(self.lib.wn_teacher_set_weights_workspace_bytes(self._h))
            ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_teacher_set_weights(self._h, _ptr(params), params.numel(), _ptr(up_params),
                                                        up_params.numel() if up_params is not None else 0, _ptr(ws),
                                                        nb if nb else ws.numel(), self._stream()))
        self._train_frames.clear()
        return self

    # ---- student training step on the device (the trainer is train.StudentTrainer) ----
    def iaf_stack_scopes(self):
        """scopes of the student's deconv stacks, in the order of d_encoding's leading axis"""
        if getattr(self.hp, 'use_share_deconv', False):
            return ['iaf_share']
        return ['iaf_{:d}'.format(k + 1) for k in range(self.iaf_n_stacks())]

    def iaf_set_weights(self, params, up_params=None):
        """Re-pack this finalized student's weights in place from flat float32 device buffers: `params` in the layout of
        iaf_grad_table(), `up_params` {scope: buffer in the layout of deconv_grad_table(scope)} or None; a stack whose scope is
        missing keeps its packs.  The handle then holds what load_weights of the same values would have built, for generation
        in every launch form and for the training calls.  Synchronises the current stream once (the scales' maxima are read
        back); tapes written before the call are refused afterwards.  A switch: RuntimeError (WN_ESTATE) while another
        thread's work call is inside the library."""
        _flat_f32('iaf_set_weights', 'params', params)
        up_params = dict(up_params or {})
        scopes = self.iaf_stack_scopes()
        unknown = sorted(set(up_params) - set(scopes))
        if unknown:
            raise ValueError('iaf_set_weights: no deconv stack with scope {} (the student has {})'.format(unknown, scopes))
        for scope, t in up_params.items():
            _flat_f32('iaf_set_weights', 'up_params[{!r}]'.format(scope), t)
        n_up = len(scopes) if up_params else 0
        ptrs = (ctypes.c_void_p * max(n_up, 1))(*[up_params[s].data_ptr() if s in up_params else None for s in scopes[:n_up]])
        sizes = (ctypes.c_size_t * max(n_up, 1))(*[up_params[s].numel() if s in up_params else 0 for s in scopes[:n_up]])
        with torch.cuda.device(self.device):
            nb = int(self.lib.wn_iaf_set_weights_workspace_bytes(self._h))
            ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)
            self._check(self.lib.wn_iaf_set_weights(self._h, _ptr(params), params.numel(), ptrs, sizes, n_up, _ptr(ws),
                                                    nb if nb else ws.numel(), self._stream()))
        self._train_frames.clear()
        return self

    def iaf_grad_floats(self):
        """floats of the flat buffer iaf_grad_table() lays out (0 for a model the training calls refuse)"""
        return int(self.lib.wn_iaf_grad_floats(self._h))

    def teacher_grad_floats(self):
        """floats of the flat buffer teacher_grad_table() lays out"""
        return int(self.lib.wn_teacher_grad_floats(self._h))

    def deconv_grad_floats(self, scope=''):
        """floats of the flat buffer deconv_grad_table(scope) lays out (0 for a stack deconv_backward refuses)"""
        return int(self.lib.wn_deconv_grad_floats(self._h, scope.encode()))

    def grad_sumsq(self, g, acc=None, accumulate=False):
        """Sum of squares of the flat float32 device tensor g as one float64 device value (fixed order, no atomics): written
        into `acc` ([1] float64) or added to it with accumulate.  Returns acc."""
        return grad_sumsq(g, acc, accumulate)

    def grad_combine(self, rows, out=None):
        """The mean of the S rows of a [S, n] float32 device tensor, summed strictly left to right in float32:
        into `out` ([n], may be rows[0]) or a new tensor.  Returns out."""
        return grad_combine(rows, out)

    def adam_ema_step(self, p, g, m, v, ema, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay_t=0.0, sumsq=None,
                      clip_norm=1.0):
        """One Adam step in place on flat float32 device tensors, with the EMA shadow (or None) and, with `sumsq` (the [1]
        float64 of grad_sumsq), tf.clip_by_global_norm(., clip_norm) applied to g on the device."""
        return adam_ema_step(p, g, m, v, ema, lr_t, beta1, beta2, eps, ema_decay_t, sumsq, clip_norm)

    def _fac(self, fac):
        fac = fac.to(device=self.device, dtype=torch.float64).contiguous()
        if fac.numel() != 2:
            raise ValueError('fac must hold two values (d loss / d sums)')
        return fac

    def distill_mol_xent_grad(self, out_params, mean_tot, scale_tot, num_samples, fac, noise=None, seed=0):
        """Gradient of fac[0] sums[0] + fac[1] sums[1] of distill_mol_xent (same draws) -> (d out_params, d mean_tot,
        d scale_tot).  fac: two float64 values on the device."""
        out_params, mean_tot, scale_tot = self._distill_args('distill_mol_xent_grad', out_params, mean_tot, scale_tot)
        B, T, S = int(mean_tot.shape[0]), int(mean_tot.shape[1]), int(num_samples)
        noise = self._dev(noise)
        if noise is not None and tuple(noise.shape) != (B, S, T):
            raise ValueError('distill_mol_xent_grad: noise must be [B, num_samples, T] = [{}, {}, {}]'.format(B, S, T))
        fac = self._fac(fac)
        d_te, d_m, d_s = torch.empty_like(out_params), torch.empty_like(mean_tot), torch.empty_like(scale_tot)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_distill_mol_xent_grad(self._h, _ptr(out_params), int(out_params.shape[2]), _ptr(mean_tot),
                                                          _ptr(scale_tot), B, T, S, _ptr(noise),
                                                          ctypes.c_uint64(seed & (2 ** 64 - 1)), _ptr(fac), _ptr(d_te),
                                                          _ptr(d_m), _ptr(d_s), self._stream()))
        return d_te, d_m, d_s

    def distill_gauss_kl_grad(self, out_params, mean_tot, scale_tot, fac):
        """Gradient of fac[0] sums[0] + fac[1] sums[1] of distill_gauss_kl -> (d out_params, d mean_tot, d scale_tot)."""
        out_params, mean_tot, scale_tot = self._distill_args('distill_gauss_kl_grad', out_params, mean_tot, scale_tot)
        B, T = int(mean_tot.shape[0]), int(mean_tot.shape[1])
        fac = self._fac(fac)
        d_te, d_m, d_s = torch.empty_like(out_params), torch.empty_like(mean_tot), torch.empty_like(scale_tot)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_distill_gauss_kl_grad(self._h, _ptr(out_params), int(out_params.shape[2]), _ptr(mean_tot),
                                                          _ptr(scale_tot), B, T, _ptr(fac), _ptr(d_te), _ptr(d_m), _ptr(d_s),
                                                          self._stream()))
        return d_te, d_m, d_s

    def iaf_cond_hoisted(self, batch, num_frames):
        """True when iaf_generate(batch, num_frames) runs the hoisted-conditioning kernels."""
        return bool(self.lib.wn_iaf_cond_hoisted(self._h, int(batch), int(num_frames)))

    def iaf_layer_groups(self, batch, num_frames):
        """True when iaf_generate(batch, num_frames) runs the residual layers in LDS-resident layer groups."""
        return bool(self.lib.wn_iaf_layer_groups(self._h, int(batch), int(num_frames)))

    def set_layer_groups(self, mode):
        """Launch structure of the hoisted form: True / 1 = layer groups wherever they apply, False / -1 = one launch per
        layer (pair), None / 0 = what the engine was created with: the library's size policy, or the form WN_GROUPS /
        WN_NO_GROUPS named then (wn_iaf_set_groups).  A switch: raises RuntimeError (WN_ESTATE) while another thread's
        generate call is inside the library."""
        m = 0 if mode is None else (1 if mode is True else -1 if mode is False else int(mode))
        self._check(self.lib.wn_iaf_set_groups(self._h, m))
        return self

    # ---- measurement aid (bench.py) ----
    def profile_begin(self):
        self._check(self.lib.wn_profile_begin(self._h))

    def profile_pause(self, paused):
        self._check(self.lib.wn_profile_pause(self._h, 1 if paused else 0))

    def profile_end(self):
        """-> (summed ms of the bracketed residual-layer kernel runs, number of launches)."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._check(self.lib.wn_profile_end(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    PROFILE_PARTS = ('prologue_epilogue', 'upsampler', 'cond_gemm', 'residual_stack')

    def profile_parts_begin(self):
        self._check(self.lib.wn_profile_parts_begin(self._h))

    def profile_parts_only(self, mask):
        """Power measurements only, and only between profile_parts_begin() and profile_parts_end() (which disarms it): run
        just the parts whose bits are set (bit k = PROFILE_PARTS[k]; 15 = everything)."""
        self._check(self.lib.wn_profile_parts_only(self._h, int(mask)))

    def profile_parts_end(self):
        """-> ({part: summed ms}, calls): HIP events at the part boundaries of every iaf_generate since parts_begin."""
        ms = (ctypes.c_double * len(self.PROFILE_PARTS))()
        n = ctypes.c_int64(0)
        self._check(self.lib.wn_profile_parts_end(self._h, ms, ctypes.byref(n)))
        return {k: ms[i] for i, k in enumerate(self.PROFILE_PARTS)}, n.value

    # ---- AR path ----
    def ar_n_rand(self):
        return int(self.lib.wn_ar_n_rand(self._h))

    def ar_new_state(self, B):
        n = self.lib.wn_ar_state_bytes(self._h, int(B))
        if n == 0:
            raise ValueError('not a finalized teacher engine')
        st = torch.empty(int(n), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_ar_reset(self._h, _ptr(st), int(B), self._stream()))
        return st

    def _check_rnd(self, rnd, shape, what):
        if rnd is not None and tuple(rnd.shape) != shape:
            raise ValueError('{}: rnd must be {}, got {}'.format(what, shape, tuple(rnd.shape)))

    def ar_step(self, state, wav_in, enc_t, rnd=None, seed=0, want_out=False):
        """One Fastgen.sample step.  wav_in [B] or [B,1]; enc_t [B,deconv_width]; rnd [B, ar_n_rand()]."""
        wav_in = self._dev(wav_in).reshape(-1)
        enc_t = self._dev(enc_t)
        B = int(wav_in.shape[0])
        if enc_t.dim() != 2 or tuple(enc_t.shape) != (B, int(self.hp.deconv_width)):
            raise ValueError('ar_step: encoding must be [{}, {}], got {}'.format(B, self.hp.deconv_width, tuple(enc_t.shape)))
        if not isinstance(state, torch.Tensor) or state.numel() != int(self.lib.wn_ar_state_bytes(self._h, B)):
            raise ValueError('ar_step: state was not created by ar_new_state({})'.format(B))
        rnd = self._dev(rnd)
        if rnd is not None and rnd.dim() == 1:
            rnd = rnd.reshape(B, -1)
        self._check_rnd(rnd, (B, self.ar_n_rand()), 'ar_step')
        sample = torch.empty((B,), dtype=torch.int32, device=self.device)
        outp = torch.empty((B, cfg.teacher_out_width(self.hp)), dtype=torch.float32, device=self.device) \
            if want_out else None
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_ar_step(self._h, _ptr(state), B, _ptr(wav_in), _ptr(enc_t), _ptr(rnd),
                                            ctypes.c_uint64(int(seed)), _ptr(sample), _ptr(outp), self._stream()))
        return (sample, outp) if want_out else sample

    def ar_cond_vars(self, enc):
        """Fastgen.cond_vars (wavenet.py:353-377): enc [B,Tn,deconv_width] -> {'mel_cond_1': [B,Tn,gate_width], ...,
        'mel_cond_<num_layers>': ..., 'mel_cond_out1': [B,Tn,skip_width]}, every layer's conditioning projection (bias
        included) in bulk over time.  The tensors are views of one device buffer."""
        enc = self._dev(enc)
        if enc.dim() != 3 or int(enc.shape[2]) != int(self.hp.deconv_width):
            raise ValueError('ar_cond_vars: enc must be [batch, steps, {}], got {}'.format(self.hp.deconv_width, tuple(enc.shape)))
        B, Tn = int(enc.shape[0]), int(enc.shape[1])
        G, S, NL = cfg.teacher_gate_width(self.hp), int(self.hp.skip_width), int(self.hp.num_layers)
        n = int(self.lib.wn_ar_cond_vars_floats(self._h, B, Tn))
        if n != B * Tn * (NL * G + S):
            raise ValueError('ar_cond_vars: needs a teacher engine and B, Tn >= 1')
        buf = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.wn_ar_cond_vars(self._h, _ptr(enc), B, Tn, _ptr(buf), self._stream()))
        out = {}
        for i in range(NL):
            out['mel_cond_%d' % (i + 1)] = buf[i * B * Tn * G:(i + 1) * B * Tn * G].view(B, Tn, G)
        out['mel_cond_out1'] = buf[NL * B * Tn * G:].view(B, Tn, S)
        return out

    def _set_ar_graph(self, on):
        """wn_ar_set_graph is a SWITCH of the shared handle (refused while another caller's work call is in flight): flipped
        only when the wanted state differs from the one the engine and its forks last set."""
        on = bool(on)
        if self._shared['ar_graph'] is not on:
            self._check(self.lib.wn_ar_set_graph(self._h, 1 if on else 0))
            self._shared['ar_graph'] = on

    def ar_generate(self, enc, rnd=None, seed=0, forced_wav=None, want_out=False, use_graph=False, streams=1):
        """fastgen.synthesis loop.  enc [B,Tn,deconv_width], rnd [Tn,B,ar_n_rand()] or None (drawn on the
        device), forced_wav [B,Tn] or None -> dict(idx, wav[, out_params]).
        The loop is a static sequence of kernels per step (every per-step address is derived on the device).
        Default: plain launches on the caller's stream.  use_graph=True replays it from hipGraphs (16 steps per
        graph); a graph cannot be captured on the legacy null stream PyTorch uses by default, so that form runs
        on a side stream of its own, ordered after and joined back into the caller's current stream.  Measured
        on MI355X the two are equally fast (191 vs 193 us per step at one utterance: the dependent-kernel chain
        on the GPU is the bound, not launch submission) and the capture costs ~20 ms per call, hence the default.

        streams=G > 1: the batch is cut into G contiguous groups of utterances, each an independent chain with its own
        queue state on its own stream, all against the one shared handle (utterances never interact: wavenet.py:379-514
        has no cross-batch term, so the results are those of the single-stream call row for row).  A step is ~65
        dependent launches of a few microseconds of work each and leaves the GPU idle in between; chains on other streams
        fill those gaps.  Each group replays hipGraphs (cheap to enqueue from one host thread), whatever use_graph says."""
        enc = self._dev(enc)
        if enc.dim() != 3 or int(enc.shape[2]) != int(self.hp.deconv_width):
            raise ValueError('ar_generate: enc must be [batch, steps, {}], got {}'.format(self.hp.deconv_width, tuple(enc.shape)))
        B, Tn = int(enc.shape[0]), int(enc.shape[1])
        rnd = self._dev(rnd)
        self._check_rnd(rnd, (Tn, B, self.ar_n_rand()), 'ar_generate')
        forced = self._dev(forced_wav)
        if forced is not None and tuple(forced.shape) != (B, Tn):
            raise ValueError('ar_generate: forced_wav must be [{}, {}], got {}'.format(B, Tn, tuple(forced.shape)))
        G = int(streams)
        if G < 1 or G > B:
            raise ValueError('ar_generate: streams must be in 1..batch ({}), got {}'.format(B, streams))
        if G > 1:
            return self._ar_generate_streams(enc, rnd, seed, forced, want_out, G)
        idx = torch.empty((B, Tn), dtype=torch.int32, device=self.device)
        wav = torch.empty((B, Tn), dtype=torch.float32, device=self.device)
        outp = torch.empty((B, Tn, cfg.teacher_out_width(self.hp)), dtype=torch.float32, device=self.device) \
            if want_out else None
        with torch.cuda.device(self.device):
            nb = self.lib.wn_ar_state_bytes(self._h, B)
            ws = self._workspace(nb)
            cur = torch.cuda.current_stream(self.device)
            self._set_ar_graph(use_graph)
            if use_graph:
                if self._ar_stream is None:
                    self._ar_stream = torch.cuda.Stream(self.device)
                run = self._ar_stream
                run.wait_stream(cur)
            else:
                run = cur
            self._check(self.lib.wn_ar_generate(
                self._h, _ptr(enc), B, Tn, _ptr(rnd), ctypes.c_uint64(int(seed)), _ptr(idx), _ptr(wav),
                _ptr(forced), _ptr(outp), _ptr(ws), ws.numel(), ctypes.c_void_p(run.cuda_stream)))
            if use_graph:
                cur.wait_stream(run)
        out = {'idx': idx, 'wav': wav}
        if want_out:
            out['out_params'] = outp
        return out

    def _ar_generate_streams(self, enc, rnd, seed, forced, want_out, G):
        B, Tn = int(enc.shape[0]), int(enc.shape[1])
        ow = cfg.teacher_out_width(self.hp)
        if self._ar_groups is None or len(self._ar_groups) < G:
            self._ar_groups = [{'stream': torch.cuda.Stream(self.device), 'ws': None} for _ in range(G)]
        bounds = [B * g // G for g in range(G + 1)]
        parts = []
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            self._set_ar_graph(True)
            for g in range(G):
                lo, hi = bounds[g], bounds[g + 1]
                nb_ = hi - lo
                grp = self._ar_groups[g]
                need = int(self.lib.wn_ar_state_bytes(self._h, nb_))
                if grp['ws'] is None or grp['ws'].numel() < need:
                    grp['ws'] = torch.empty(need, dtype=torch.uint8, device=self.device)
                # per-group inputs / outputs are contiguous tensors of their own (the C ABI takes dense [b, Tn, ...] arrays)
                e = enc[lo:hi].contiguous()
                r = rnd[:, lo:hi].contiguous() if rnd is not None else None
                f = forced[lo:hi].contiguous() if forced is not None else None
                idx = torch.empty((nb_, Tn), dtype=torch.int32, device=self.device)
                wav = torch.empty((nb_, Tn), dtype=torch.float32, device=self.device)
                outp = torch.empty((nb_, Tn, ow), dtype=torch.float32, device=self.device) if want_out else None
                parts.append((e, r, f, idx, wav, outp))
            for g in range(G):
                self._ar_groups[g]['stream'].wait_stream(cur)
            for g in range(G):
                e, r, f, idx, wav, outp = parts[g]
                grp = self._ar_groups[g]
                # device-drawn randoms: every group draws from its own Philox key (seed + group); injected randoms are
                # the caller's columns lo..hi, so the result is the single-stream call's row for row
                self._check(self.lib.wn_ar_generate(
                    self._h, _ptr(e), int(e.shape[0]), Tn, _ptr(r), ctypes.c_uint64(int(seed) + g), _ptr(idx), _ptr(wav),
                    _ptr(f), _ptr(outp), _ptr(grp['ws']), grp['ws'].numel(), ctypes.c_void_p(grp['stream'].cuda_stream)))
            for g in range(G):
                cur.wait_stream(self._ar_groups[g]['stream'])
            # (every tensor above was allocated on `cur`, the side streams start behind it and are joined back into it:
            # the caching allocator can only hand their memory to work that `cur` orders behind the joins)
        out = {'idx': torch.cat([p[3] for p in parts], 0), 'wav': torch.cat([p[4] for p in parts], 0)}
        if want_out:
            out['out_params'] = torch.cat([p[5] for p in parts], 0)
        return out


class IafStream(object):
    """Audio while the mel frames are still arriving (Engine.iaf_stream).

    push(mel_frames [B,n,n_mel]) -> dict of the samples that became final ([B,m] per name in `want`, m >= 0), finish() ->
    the tail, close().  The concatenation of everything returned equals
    engine.iaf_generate_long(all_mel, seed=seed, crop='left', window_frames=window_frames) bit for bit however the frames
    were cut into pushes: windows sit on the fixed grid of config.iaf_plan_windows, a grid window runs as soon as more
    than its last frame has arrived (so it cannot turn out to be the tail), and finish() plans what is left with the frame
    count then known.  crop='left' is the one-shot's centred crop whenever the total frame count is a multiple of
    `period`.  A window is window_frames long, so the first samples appear after about that many frames.

    The stream is a caller of its own in the sense of Engine.fork(): it shares the engine's weights, owns its workspace
    and the trailing mel frames it still needs (on the device), and issues its work on the torch stream current in the
    calling thread; one stream object belongs to one thread, and the engine must outlive it."""

    def __init__(self, engine, batch=1, seed=0, window_frames=None, want=('wav',)):
        self.eng = engine.fork()
        self.B, self.seed, self.want = int(batch), int(seed), tuple(want)
        if self.B < 1:
            raise ValueError('iaf_stream: batch must be >= 1')
        hp = self.eng.hp
        self.window_frames = int(window_frames) if window_frames is not None else cfg.iaf_default_window_frames(hp)
        self.Fw, _, self.lo, self.S = cfg.iaf_window_grid(hp, self.window_frames, 0)
        self._mel = None          # frames self._base .. self.frames of every utterance, [B, n, n_mel] on the device
        self._base = 0
        self.frames = 0           # frames pushed so far
        self._next = 0            # next grid window
        self.samples = 0          # samples returned so far
        self._closed = False

    def _run(self, rows, n_out):
        """rows (f0, t_origin, keep_from, keep_to, out_t) of the utterance plan -> the n_out samples behind self.samples"""
        eng = self.eng
        out = eng._window_outputs(self.B, n_out, self.want)
        if n_out > 0:
            Fw = rows[0][5]
            mel_rows = torch.stack([self._mel[b, f0 - self._base:f0 - self._base + Fw] for (f0, *_r) in rows
                                    for b in range(self.B)])
            # the noise is absolute (t_origin); only the place in the returned chunk is relative
            desc = [(b, to, kf, kt, ot - self.samples) for (f0, to, kf, kt, ot, _) in rows for b in range(self.B)]
            eng.iaf_generate_windows(mel_rows, desc, out, None, self.seed, None, 1, True)
            self.samples += n_out
        return {k: v for k, v in out.items() if k in self.want}

    def push(self, mel_frames):
        if self._closed:
            raise RuntimeError('iaf_stream: push after finish() / close()')
        eng = self.eng
        m = eng._dev(mel_frames)
        if m.dim() != 3 or int(m.shape[0]) != self.B or int(m.shape[2]) != eng.n_mel:
            raise ValueError('mel_frames must be [{}, n, {}], got {}'.format(self.B, eng.n_mel, tuple(m.shape)))
        self._mel = m if self._mel is None else torch.cat([self._mel, m], 1)
        self.frames += int(m.shape[1])
        fs, rows, n_out = eng.frame_shift, [], 0
        while self.frames > self._next * self.S + self.Fw:         # certain to be a grid window of the final plan
            f0 = self._next * self.S
            to, kt = f0 * fs, self.lo + self.S * fs
            kf = self.samples + n_out - to
            rows.append((f0, to, kf, kt, self.samples + n_out, self.Fw))
            n_out += kt - kf
            self._next += 1
        out = self._run(rows, n_out)
        # the tail window starts behind the last grid window that ran: frames before that one are not needed again
        keep_from = max(self._next - 1, 0) * self.S
        if keep_from > self._base:
            self._mel = self._mel[:, keep_from - self._base:].contiguous()
            self._base = keep_from
        return out

    def finish(self):
        """The samples not returned yet; the stream is closed afterwards."""
        if self._closed:
            raise RuntimeError('iaf_stream: finish after finish() / close()')
        rows, n_out = [], 0
        if self.frames > 0 and self.eng.iaf_length(self.frames) > 0:
            Fw, plan = cfg.iaf_plan_windows(self.eng.hp, self.frames, self.window_frames, 'left')
            assert self._next == 0 or (Fw == self.Fw and self._next == len(plan) - 1), (Fw, self.Fw, self._next, len(plan))
            rows = [r + (Fw,) for r in plan[self._next:]]
            n_out = self.eng.iaf_length(self.frames) - self.samples
        out = self._run(rows, n_out)
        self.close()
        return out

    def close(self):
        self._closed = True
        self._mel = None
        self.eng.close()


PRIORITY_FREQ = 384        # auxilaries/mel_extractor.py:27 (bins below 3 kHz)
STFT_BINS = 1025
STFT_HOP = 200


def _trim(x, trim_len):
    """ParallelWavenet._trim (parallel_wavenet.py:431-436): drop trim_len samples, trim_len // 2 of them on the left -- a view."""
    left = int(trim_len // 2)
    return x[:, left:left + int(x.shape[1]) - int(trim_len)]


def power_loss(pred, orig, device=None):
    """ParallelWavenet.power_loss (parallel_wavenet.py:459-479) on the device, with the reference's module constants:
    pred, orig [B,L] audio (device tensors or arrays); the longer one is centre-trimmed to the shorter.  Returns the loss,
    0.5 mean (|P| - |O|)^2 + 0.5 of the same over the bins below 3 kHz, as a 0-d float64 device tensor."""
    lib = _lib.load()
    dev = torch.device(device) if device is not None else (pred.device if isinstance(pred, torch.Tensor) and pred.is_cuda
                                                             else torch.device('cuda', torch.cuda.current_device()))

    def to_dev(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.float32)
        return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)
    pred, orig = to_dev(pred), to_dev(orig)
    if pred.dim() != 2 or orig.dim() != 2 or pred.shape[0] != orig.shape[0]:
        raise ValueError('power_loss: pred and orig must be [B,L] with equal B')
    pred = pred if pred.stride(1) == 1 else pred.contiguous()
    orig = orig if orig.stride(1) == 1 else orig.contiguous()
    lp, lo = int(pred.shape[1]), int(orig.shape[1])
    if lp > lo:
        pred = _trim(pred, lp - lo)
    elif lo > lp:
        orig = _trim(orig, lo - lp)
    B, L = int(pred.shape[0]), int(pred.shape[1])
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(lib.wn_power_loss_workspace_bytes(B, L)), 256), dtype=torch.uint8, device=dev)
        _lib.check(lib.wn_power_loss(_ptr(pred), pred.stride(0), _ptr(orig), orig.stride(0), B, L, _ptr(out), _ptr(ws),
                                     ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    nf = (L + STFT_HOP - 1) // STFT_HOP
    return 0.5 * out[0] / (B * nf * STFT_BINS) + 0.5 * out[1] / (B * nf * PRIORITY_FREQ)


def power_loss_sums(pred, orig):
    """wn_power_loss on two device rows [B,L] of equal length (unit inner stride): the two float64 sums of power_loss."""
    lib = _lib.load()
    dev = pred.device
    B, L = int(pred.shape[0]), int(pred.shape[1])
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(lib.wn_power_loss_workspace_bytes(B, L)), 256), dtype=torch.uint8, device=dev)
        _lib.check(lib.wn_power_loss(_ptr(pred), pred.stride(0), _ptr(orig), orig.stride(0), B, L, _ptr(out), _ptr(ws),
                                     ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


def power_loss_grad(pred, orig, fac):
    """Gradient of fac[0] out2[0] + fac[1] out2[1] of power_loss_sums(pred, orig) with respect to pred -> [B,L] float32."""
    lib = _lib.load()
    dev = pred.device
    B, L = int(pred.shape[0]), int(pred.shape[1])
    fac = fac.to(device=dev, dtype=torch.float64).contiguous()
    d = torch.empty((B, L), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(lib.wn_power_loss_grad_workspace_bytes(B, L)), 256), dtype=torch.uint8, device=dev)
        _lib.check(lib.wn_power_loss_grad(_ptr(pred), pred.stride(0), _ptr(orig), orig.stride(0), B, L, _ptr(fac), _ptr(d),
                                          d.stride(0), _ptr(ws), ws.numel(),
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return d


def _flat_f32(what, name, t, n=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous()):
        raise ValueError('{}: {} must be a flat contiguous float32 device tensor'.format(what, name))
    if n is not None and t.numel() != n:
        raise ValueError('{}: {} holds {} values, not {}'.format(what, name, t.numel(), n))
    return t


def grad_sumsq(g, acc=None, accumulate=False):
    """wn_grad_sumsq: the sum of squares of a flat float32 device tensor in float64, as a [1] float64 device tensor (`acc`,
    or a new one); accumulate adds to acc instead of overwriting it."""
    lib = _lib.load()
    g = _flat_f32('grad_sumsq', 'g', g)
    if g.numel() < 1:
        raise ValueError('grad_sumsq: g is empty')
    dev = g.device
    if acc is None:
        if accumulate:
            raise ValueError('grad_sumsq: accumulate needs acc')
        acc = torch.empty(1, dtype=torch.float64, device=dev)
    elif not (acc.is_cuda and acc.dtype == torch.float64 and acc.numel() == 1):
        raise ValueError('grad_sumsq: acc must be one float64 value on the device')
    with torch.cuda.device(dev):
        nb = int(lib.wn_grad_sumsq_workspace_bytes(g.numel()))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        _lib.check(lib.wn_grad_sumsq(_ptr(g), g.numel(), _ptr(acc), 1 if accumulate else 0, _ptr(ws), nb,
                                     ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return acc


GRAD_COMBINE_MAX_ROWS = 64


def grad_combine(rows, out=None):
    """wn_grad_combine: out[i] = (((rows[0, i] + rows[1, i]) + ...) + rows[S - 1, i]) * float32(1 / S), in float32 and in
    that order (train.combine_np is the numpy twin).  rows: a [S, n] float32 device tensor, 1 <= S <= 64, with unit inner
    stride and a row stride >= n (a view of a wider buffer will do); out: a flat float32 device tensor of n values with unit
    stride, rows[0] itself or memory outside rows (None: a new one).  Returns out."""
    lib = _lib.load()
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2):
        raise ValueError('grad_combine: rows must be a [S, n] float32 device tensor')
    S, n = int(rows.shape[0]), int(rows.shape[1])
    if not 1 <= S <= GRAD_COMBINE_MAX_ROWS:
        raise ValueError('grad_combine: {} rows; the combine takes 1 to {}'.format(S, GRAD_COMBINE_MAX_ROWS))
    if n < 1:
        raise ValueError('grad_combine: rows are empty')
    stride = int(rows.stride(0)) if S > 1 else n
    if rows.stride(1) != 1 or stride < n:
        raise ValueError('grad_combine: rows need unit inner stride and a row stride >= n, got strides {}'.format(tuple(rows.stride())))
    dev = rows.device
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32 and out.dim() == 1
              and out.numel() == n and (n == 1 or out.stride(0) == 1)):
        raise ValueError('grad_combine: out must be a flat float32 tensor of {} values on the device of rows'.format(n))
    lo, hi = out.data_ptr(), out.data_ptr() + 4 * n
    r0 = rows.data_ptr()
    if lo != r0 and lo < r0 + 4 * ((S - 1) * stride + n) and hi > r0:
        raise ValueError('grad_combine: out overlaps rows (only rows[0] itself may be the output)')
    with torch.cuda.device(dev):
        _lib.check(lib.wn_grad_combine(_ptr(rows), n, stride, S, _ptr(out),
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


def adam_ema_step(p, g, m, v, ema, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay_t=0.0, sumsq=None, clip_norm=1.0):
    """wn_adam_ema_step in place on flat float32 device tensors of equal length (ema may be None; sumsq: None or the [1]
    float64 squared global norm, which turns the clip on)."""
    lib = _lib.load()
    p = _flat_f32('adam_ema_step', 'p', p)
    n = p.numel()
    if n < 1:
        raise ValueError('adam_ema_step: p is empty')
    for name, t in (('g', g), ('m', m), ('v', v)) + ((('ema', ema),) if ema is not None else ()):
        _flat_f32('adam_ema_step', name, t, n)
    if sumsq is not None and not (sumsq.is_cuda and sumsq.dtype == torch.float64 and sumsq.numel() == 1):
        raise ValueError('adam_ema_step: sumsq must be one float64 value on the device')
    dev = p.device
    with torch.cuda.device(dev):
        _lib.check(lib.wn_adam_ema_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), n, float(lr_t), float(beta1),
                                        float(beta2), float(eps), float(ema_decay_t), _ptr(sumsq), float(clip_norm),
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return p
