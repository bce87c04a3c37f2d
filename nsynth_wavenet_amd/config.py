"""Config surface: the reference's config_jsons/*.json read into an
argparse.Namespace exactly like eval_wavenet.py:28-30 does, plus the
per-class `getattr` defaults the reference scatters through its model classes
(wavenet.py:105-129,326-345; parallel_wavenet.py:124-141), gathered in one place.
Training-only keys are accepted and ignored."""
import json
from argparse import Namespace

from . import _lib


def load_hparams(path_or_dict):
    if isinstance(path_or_dict, Namespace):
        return path_or_dict
    if isinstance(path_or_dict, dict):
        return Namespace(**path_or_dict)
    with open(path_or_dict, 'rt') as f:
        return Namespace(**json.load(f))


def model_kind(hparams):
    """'student' (ParallelWavenet) when the JSON has num_iaf_layers, else 'teacher'."""
    return 'student' if hasattr(hparams, 'num_iaf_layers') else 'teacher'


def quant_chann(hparams):
    return 2 ** 8 if hparams.use_mu_law else 2 ** 16     # wavenet.py:117-120


def teacher_gate_width(hparams):
    # double_gate_width defaults to TRUE when the key is absent (wavenet.py:106,329)
    return 2 * hparams.width if getattr(hparams, 'double_gate_width', True) else hparams.width


def teacher_out_width(hparams):
    lt = hparams.loss_type                                # wavenet.py:121-129
    if lt == 'ce':
        return quant_chann(hparams)
    if lt == 'mol':
        return hparams.mol_mix * 3
    if lt == 'gauss':
        return 2
    raise ValueError('[{}] loss is not supported'.format(lt))


def frame_shift(hparams):
    fs = 1
    for _, s in hparams.deconv_config:
        fs *= s
    return fs


def iaf_length(hparams, num_frames):
    """parallel_wavenet.py:293-302."""
    md = 2 ** (hparams.num_stages - 1)
    return (num_frames * frame_shift(hparams) // md) * md


# name -> (wn_config.precision, wn_config.cond_mode)
PRECISIONS = {'f16x3': (0, 0), 'f16x3-fused': (0, 1), 'f16x3-hoisted': (0, 2), 'f32': (1, 0), 'f32-fused': (1, 1), 'f32-hoisted': (1, 2)}


def default_precision():
    """IAF contraction arithmetic: 'f16x3' = split-fp16 operands on the fp16 MFMA (three MFMAs per
    product, ~22-bit operands, fp32 accumulate) -- the default; it hoists the per-layer
    conditioning 1x1s into one GEMM per deconv stack and runs the small-dilation layers two per
    launch ('f16x3-hoisted' names that form explicitly; 'f16x3-fused' evaluates the 1x1s inside
    every layer kernel instead and needs no conditioning workspace); 'f32' = fp32 MFMA, the reference's own
    arithmetic -- since round 6 with the same split: the conditioning 1x1s in one fp32 GEMM per deconv stack and the residual
    layers on the dilated conv alone ('f32-hoisted' names that form, 'f32-fused' the one kernel per layer that reads enc itself)."""
    import os
    return os.environ.get('WN_PRECISION', 'f16x3')


def to_wn_config(hparams, kind=None, n_mel=80, precision=None):
    kind = kind or model_kind(hparams)
    c = _lib.WnConfig()
    precision = precision or default_precision()
    if precision not in PRECISIONS:
        raise ValueError('precision must be one of {}'.format(sorted(PRECISIONS)))
    c.precision, c.cond_mode = PRECISIONS[precision]
    c.use_resize_conv = int(bool(getattr(hparams, 'use_resize_conv', False)))
    dc = hparams.deconv_config
    if len(dc) > _lib.WN_MAX_DECONV:
        raise ValueError('deconv_config has too many layers')
    c.n_mel = n_mel
    c.width = hparams.width
    c.deconv_width = hparams.deconv_width
    c.n_deconv = len(dc)
    for j, (fl, s) in enumerate(dc):
        c.deconv_filter[j] = fl
        c.deconv_stride[j] = s
    c.filter_length = hparams.filter_length
    c.num_stages = hparams.num_stages
    c.use_mu_law = int(bool(hparams.use_mu_law))
    c.use_weight_norm = int(bool(getattr(hparams, 'use_weight_norm', False)))
    c.upsample_act = _lib.ACT[getattr(hparams, 'upsample_act', 'tanh')]   # default 'tanh' (wavenet.py:108)
    if kind == 'student':
        share = bool(getattr(hparams, 'use_share_deconv', False))
        teach = bool(getattr(hparams, 'use_teacher_deconv', False))
        if share and teach:
            raise ValueError('use_share_deconv and use_teacher_deconv are mutually exclusive')  # :135
        lt = getattr(hparams, 'loss_type', 'logistic')
        if lt not in ('logistic', 'gauss'):
            raise ValueError('student loss_type must be logistic or gauss')
        if len(hparams.num_iaf_layers) > _lib.WN_MAX_FLOWS:
            raise ValueError('too many IAF flows')
        c.kind = _lib.KIND_STUDENT
        c.gate_width = hparams.width                       # parallel_wavenet.py:209
        c.n_flows = len(hparams.num_iaf_layers)
        for k, n in enumerate(hparams.num_iaf_layers):
            c.iaf_layers[k] = n
        c.loss_type = _lib.LOSS[lt]
        c.out_width = 2
        c.share_deconv = int(share or teach)
    else:
        c.kind = _lib.KIND_TEACHER
        c.skip_width = hparams.skip_width
        c.gate_width = teacher_gate_width(hparams)
        c.num_layers = hparams.num_layers
        c.loss_type = _lib.LOSS[hparams.loss_type]
        c.mol_mix = getattr(hparams, 'mol_mix', 0) if hparams.loss_type == 'mol' else 0
        c.out_width = teacher_out_width(hparams)
    return c


# ---- windowed IAF generation: geometry and the window planner; wn_iaf_window_geometry is the C twin ----
def _deconv_frame_span(hparams):
    """(frames_before, frames_after): frames left / right of the frame that holds an enc column which reach that column
    through the deconv stack.  One layer maps the output interval [a, b] onto the inputs it reads --
    trans conv (filter K, stride s, pL = max(K - s, 0) // 2): y[n] reads x[i] for 0 <= n + pL - i s < K,
        i in [ceil((a + pL - K + 1) / s), floor((b + pL) / s)];
    resize conv (pl = (K - 1) // 2): y[n] reads the repeated input at n - pl .. n - pl + K - 1,
        i in [floor((a - pl) / s), floor((b - pl + K - 1) / s)]
    -- and the stack is the composition, last layer first.  The stack is shift-invariant by whole frames, so the span of
    one frame far from the edges is the span of every frame."""
    fs = frame_shift(hparams)
    f = 1 << 20
    a, b = f * fs, (f + 1) * fs - 1
    resize = bool(getattr(hparams, 'use_resize_conv', False))
    for K, s in reversed(hparams.deconv_config):
        if resize:
            pl = (K - 1) // 2
            a, b = (a - pl) // s, (b - pl + K - 1) // s
        else:
            pL = max(K - s, 0) // 2
            a, b = -((-(a + pL - K + 1)) // s), (b + pL) // s
    return f - a, b - f


def iaf_window_geometry(hparams):
    """Geometry of windowed IAF generation -> Namespace(reach, frames_before, frames_after, period).

    reach: samples to the LEFT of t that x, mean_tot and scale_tot at t depend on (noise and conditioning).  One flow
    reads x[t - fl .. t - 1] in its start conv (filter_length taps on shift_right(x)) and every layer of dilation d
    widens that by (fl - 1) d, so its mean and scale at t read x[t - r_k .. t - 1], r_k = fl + (fl - 1) sum_i d_i; its
    output x[t] = x[t] scale[t] + mean[t] reads x[t - r_k .. t].  Flows chain on x, so the reaches add and nothing else
    is added: reach = sum_k r_k (12 288 for the shipped configs).
    frames_before / frames_after: see _deconv_frame_span.  period: the centre crop depends on F modulo this."""
    from math import gcd
    fl, ns = int(hparams.filter_length), int(hparams.num_stages)
    reach = 0
    for n in hparams.num_iaf_layers:
        reach += fl + (fl - 1) * sum(2 ** (i % ns) for i in range(n))
    fb, fa = _deconv_frame_span(hparams)
    md = 2 ** (ns - 1)
    return Namespace(reach=reach, frames_before=fb, frames_after=fa, period=md // gcd(frame_shift(hparams), md))


def iaf_window_margins(hparams, Fw):
    """(T_w, c0_w, lo, hi) of a row of Fw frames: its length and centre crop, and the local range [lo, hi) a row in the
    MIDDLE of an utterance may keep.  Local sample t reads the conditioning of local samples t - reach .. t, i.e. enc
    columns t - reach + c0_w .. t + c0_w of the row; a column is the utterance's own when the frames_before frames left
    and the frames_after frames right of its frame lie inside the row."""
    g = iaf_window_geometry(hparams)
    fs = frame_shift(hparams)
    Tw = iaf_length(hparams, Fw)
    c0 = (Fw * fs - Tw) // 2
    lo = g.reach + max(0, g.frames_before * fs - c0)
    hi = min(Tw, (Fw - g.frames_after) * fs - c0)
    return Tw, c0, lo, hi


def iaf_default_window_frames(hparams):
    """4.8 s windows for the shipped geometry (the one-shot's flagship shape), at least four times the recomputed part"""
    g = iaf_window_geometry(hparams)
    fs = frame_shift(hparams)
    return max(384, 4 * (-(-g.reach // fs) + g.frames_before + g.frames_after + 1))


def iaf_window_align(hparams):
    """(al, q): rows start on multiples of al frames (their first sample is a multiple of 4, the granularity of the noise
    counter) and frame counts are chosen modulo q = lcm(period, al)"""
    from math import gcd
    al = 4 // gcd(frame_shift(hparams), 4)
    p = iaf_window_geometry(hparams).period
    return al, p * al // gcd(p, al)


def iaf_window_grid(hparams, window_frames, residue):
    """The window grid for frame counts = residue (mod q): (Fw, c0_w, lo, S) with Fw the largest such count <=
    window_frames that leaves a stride S >= 1 (the smallest that does, if window_frames is too small for the geometry);
    row i of the grid starts at frame i S and keeps local [lo, lo + S frame_shift)."""
    g = iaf_window_geometry(hparams)
    fs = frame_shift(hparams)
    al, q = iaf_window_align(hparams)
    md = 2 ** (hparams.num_stages - 1)

    def stride(Fw):
        Tw, c0, lo, hi = iaf_window_margins(hparams, Fw)
        return c0, lo, (((hi - lo) // fs) // al * al if hi > lo else 0)
    Fw = int(window_frames) - (int(window_frames) - residue) % q
    if Fw < 1 or stride(Fw)[2] < 1:
        need = -(-(g.reach + (g.frames_before + g.frames_after + al + 1) * fs + md) // fs)
        Fw = need + (residue - need) % q
    c0, lo, S = stride(Fw)
    if S < 1:
        raise ValueError('iaf_window_grid: no window of {} frames fits this geometry'.format(Fw))
    return Fw, c0, lo, S


def iaf_plan_windows(hparams, F, window_frames=None, crop='centre'):
    """Plan utterance of F frames as rows of one frame count -> (Fw, [(f0, t_origin, keep_from, keep_to, out_t), ...]).

    Every row is an ordinary call on mel[f0 : f0 + Fw] (T_w = iaf_length(Fw), its own centre crop c0_w); its local sample t
    is sample t_origin + t of the utterance, it may keep local [keep_from, keep_to), and those go to out_t.. of the output.
    crop='centre': the output is iaf_generate's (T = iaf_length(F), conditioning centre-cropped); Fw = F (mod period).
    crop='left': T = floor(F frame_shift / max_dil) max_dil samples with the conditioning cropped on the right only
    (sample t reads enc column t); Fw = 0 (mod period); the same as 'centre' whenever F % period == 0.
    Fw is the largest such count <= window_frames (the smallest that leaves a row something to keep, if that is larger).

    Rows sit on a grid that does not depend on F: row i starts at frame i S and keeps local [lo, lo + S frame_shift)
    (row 0 from 0), with [lo, hi) of iaf_window_margins and S = (hi - lo) // frame_shift.  Grid rows are those that end
    before frame F; the TAIL row is placed to end at frame F and keeps what the grid rows left, up to T.  So a row that
    is certain to be a grid row (more than i S + Fw frames known) can run before F is known -- the stream does that."""
    if crop not in ('centre', 'left'):
        raise ValueError("crop must be 'centre' or 'left', got {!r}".format(crop))
    F = int(F)
    if F < 1:
        raise ValueError('iaf_plan_windows: F must be >= 1')
    fs = frame_shift(hparams)
    wf = int(window_frames) if window_frames is not None else iaf_default_window_frames(hparams)
    if wf < 1:
        raise ValueError('iaf_plan_windows: window_frames must be >= 1')
    q = iaf_window_align(hparams)[1]
    T = iaf_length(hparams, F)
    # one row: the one-shot itself ('left': only where the two crops coincide)
    if F <= wf and (crop == 'centre' or F % q == 0):
        return F, [(0, 0, 0, T, 0)]
    Fw, c0, lo, S = iaf_window_grid(hparams, min(wf, F), F % q if crop == 'centre' else 0)
    if F <= Fw:
        if F == Fw:
            return F, [(0, 0, 0, T, 0)]
        raise ValueError("iaf_plan_windows: crop='left' plans an utterance of {} frames (not a multiple of {}) as windows "
                         "of {} frames and needs at least that many".format(F, q, Fw))
    if ((F - Fw) * fs) % 4:
        raise ValueError('iaf_plan_windows: the tail window would start at sample {} (frame_shift {}): the device noise '
                         'is drawn four samples per counter'.format((F - Fw) * fs, fs))
    c0g = c0 if crop == 'centre' else 0
    rows, done, f0 = [], 0, 0
    while f0 + Fw < F:                                     # grid rows
        to = f0 * fs + c0 - c0g
        kf = done - to
        kt = lo + S * fs
        rows.append((f0, to, kf, kt, done))
        done = to + kt
        f0 += S
    f0 = F - Fw                                            # tail row: ends at frame F
    to = f0 * fs + c0 - c0g
    rows.append((f0, to, done - to, T - to, done))
    return Fw, rows
