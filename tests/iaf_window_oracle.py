"""Float64 helpers of the windowed-generation tests (not a test module): the student's feed-forward with an explicit
conditioning crop, and a window plan executed row by row with the oracle."""
import numpy as np

from oracle import wavenet_np as O

SMALL = {'width': 32, 'deconv_width': 16, 'filter_length': 3, 'num_stages': 4, 'num_iaf_layers': [5, 3],
         'deconv_config': [[8, 2], [12, 4]], 'loss_type': 'logistic', 'use_mu_law': False, 'use_share_deconv': True,
         'use_teacher_deconv': False, 'use_weight_norm': False, 'use_resize_conv': False, 'upsample_act': 'tanh'}


def feed_forward_cropped(mel, noise, weights, hp, c0, dtype=np.float64):
    """O.iaf_feed_forward with the conditioning taken from upsampled column c0 on (c0 = the centre crop gives
    O.iaf_feed_forward itself, c0 = 0 the left-aligned crop): O.deconv_stack composed with O.iaf_flow."""
    mel = np.asarray(mel, dtype)
    x0 = np.asarray(noise, dtype)
    T = x0.shape[1]
    share = hp.get('use_share_deconv', False) or hp.get('use_teacher_deconv', False)
    x = x0[:, :, None]
    mean_tot, scale_tot = np.zeros_like(x), np.ones_like(x)
    for k in range(len(hp.num_iaf_layers)):
        en = O.deconv_stack(mel, weights, hp, 'iaf_share' if share else 'iaf_{:d}'.format(k + 1), dtype)
        o = O.iaf_flow(x, en[:, c0:c0 + T], weights, hp, k, dtype)
        x = o['x']
        mean_tot = o['mean'] + mean_tot * o['scale']
        scale_tot = scale_tot * o['scale']
    mean_tot = mean_tot[:, :, 0]
    scale_tot = np.minimum(scale_tot, dtype(O.EXP_7))[:, :, 0]
    return {'x': x0 * scale_tot + mean_tot, 'mean_tot': mean_tot, 'scale_tot': scale_tot}


def run_plan(mel, noise, weights, hp, Fw, rows, dtype=np.float64):
    """Every row as an ordinary call on its Fw frames (natural layout) with the utterance's noise at its absolute
    positions (0 outside), the kept samples put at out_t: -> {'x', 'mean_tot', 'scale_tot'} [B, T], and a count of
    writers per sample."""
    B, T = noise.shape
    Tw = O.iaf_length(Fw, hp)
    out = {k: np.full((B, T), np.nan, dtype) for k in ('x', 'mean_tot', 'scale_tot')}
    writers = np.zeros(T, np.int64)
    for f0, t_origin, keep_from, keep_to, out_t in rows:
        nz = np.zeros((B, Tw), dtype)
        hi = min(T, t_origin + Tw)
        nz[:, :hi - t_origin] = noise[:, t_origin:hi]
        ff = O.iaf_feed_forward(mel[:, f0:f0 + Fw], nz, weights, hp, dtype)
        n = keep_to - keep_from
        for k in out:
            out[k][:, out_t:out_t + n] = ff[k][:, keep_from:keep_to]
        writers[out_t:out_t + n] += 1
    return out, writers
