"""tests/golden/ref_distill.npz pins itself: the distillation losses the reference's own ParallelWavenet.calculate_loss and its
parts produced (tests/golden/make_ref_distill.py) are recomputed here from the stored inputs by a float64 numpy restatement
of wavenet/parallel_wavenet.py:361-512 and wavenet/loss_func.py:22-75.  CPU only."""
import json
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
PRIORITY_FREQ = 384


def uniforms(R):
    """the [B*S, T] uniforms of kl_loss_logistic's and contrastive_loss's random nodes (make_ref_distill.uniforms)"""
    B, T = R['mol/in_x'].shape
    S = int(R['S'])
    u = np.random.RandomState(int(R['mol/u_seed'])).uniform(1e-5, 1 - 1e-5, [2, B * S, T]).astype(np.float32)
    return u[0].astype(np.float64), u[1].astype(np.float64)


def teacher_out(R, tag, mel_key):
    """the teacher's float64 out_params on the student's x (oracle.wavenet_np: float64 numpy restatement of wavenet.py)"""
    from oracle import wavenet_np as O
    cfg = json.loads(str(R[tag + '/te_cfg_json']))
    hp = O.HP(cfg)
    w = O.synth_weights(hp, 'teacher', seed=int(R[tag + '/te_seed']), init=str(R[tag + '/te_init']))
    enc = O.deconv_stack(R['{}/in_{}'.format(tag, mel_key)].astype(np.float64), w, hp, '', np.float64)
    return O.teacher_feed_forward(R[tag + '/in_x'].astype(np.float64), enc, w, hp, np.float64)


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


def _softplus(v):
    return np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))


def _sigmoid(v):
    return 0.5 * (1 + np.tanh(0.5 * v))


def mol_log_probs(par, x, Q):
    """loss_func.py:22-63 as the reference writes it: float64 difference of the two sigmoids."""
    M = par.shape[-1] // 3
    lg, mean, ls = par[..., :M], par[..., M:2 * M], np.maximum(par[..., 2 * M:], -7.0)
    inv = np.exp(-ls)
    x = x[..., None]
    c = x - mean
    plus, mn = inv * (c + 1.0 / Q), inv * (c - 1.0 / Q)
    delta = _sigmoid(plus) - _sigmoid(mn)
    max_thres, min_thres = (Q - 1 - 0.5) / (Q / 2.) - 1.0, 0.5 / (Q / 2.) - 1.0
    lp = np.where(x < min_thres, plus - _softplus(plus),
                  np.where(x > max_thres, -_softplus(mn), np.log(np.maximum(delta, 1e-12))))
    lsm = lg - lg.max(-1, keepdims=True)
    lsm = lsm - np.log(np.exp(lsm).sum(-1, keepdims=True))
    v = lp + lsm
    m = v.max(-1)
    return m + np.log(np.exp(v - m[..., None]).sum(-1))


def h_bl(te, mean, scale, u, S):
    """kl_loss_logistic's H_Ps_Pt_bl (parallel_wavenet.py:370-394): row b*S + s of the draw against row b."""
    B, T = mean.shape
    rl = (np.log(u) - np.log(1.0 - u)).reshape(B, S, T)
    x = rl * scale[:, None, :] + mean[:, None, :]
    lp = mol_log_probs(np.repeat(te[:, None], S, axis=1), x, 65536)
    return -lp.mean(axis=1)


def kl_logistic(te, mean, scale, log_scale, u, S):
    hb = h_bl(te, mean, scale, u, S)
    H_Ps = log_scale.mean() + 2
    return {'kl_loss': hb.mean() - H_Ps, 'H_Ps': H_Ps, 'H_Ps_Pt': hb.mean(), 'H_bl': hb}


def kl_gauss(te, mean_q, scale_q, log_scale_q):
    mean_p, log_scale_p = te[..., 0], np.maximum(te[..., 1], -7.0)
    scale_p = np.exp(log_scale_p)
    kl_bl = log_scale_p - log_scale_q + (scale_q ** 2 - scale_p ** 2 + (mean_p - mean_q) ** 2) / (2 * scale_p ** 2)
    return {'kl_loss': kl_bl.mean() + 4.0 * ((log_scale_p - log_scale_q) ** 2).mean(), 'kl_bl': kl_bl}


def stft_mag(y):
    """tf.contrib.signal.stft(frame_length=800, frame_step=200, fft_length=2048, pad_end=True), magnitude."""
    L = y.shape[1]
    nf = -(-L // 200)
    y = np.pad(y, [(0, 0), (0, (nf - 1) * 200 + 800 - L)])
    n = np.arange(800)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 800)
    frames = y[:, np.arange(nf)[:, None] * 200 + n[None, :]] * w
    return np.abs(np.fft.rfft(frames, n=2048, axis=-1))


def power_loss(pred, orig):
    lp, lo = pred.shape[1], orig.shape[1]
    if lp > lo:
        pred = pred[:, (lp - lo) // 2:(lp - lo) // 2 + lo]
    elif lo > lp:
        orig = orig[:, (lo - lp) // 2:(lo - lp) // 2 + lp]
    d = (stft_mag(orig) - stft_mag(pred)) ** 2
    return 0.5 * d.mean() + 0.5 * d[:, :, :PRIORITY_FREQ].mean()


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _in(R, tag, k):
    return R['{}/in_{}'.format(tag, k)].astype(np.float64)


def test_golden_shapes_and_settings(R):
    S = int(R['S'])
    assert S == 8
    hp = json.loads(str(R['mol/st_cfg_json']))
    assert hp['num_samples'] == S and hp['power_loss_factor'] > 0 and hp['contrastive_loss_factor'] > 0
    B, T = R['mol/in_x'].shape
    assert R['mol/full_H_bl'].shape == (B, T) and R['mol/in_te_out_f32'].shape == (B, T, 30)
    assert R['mol/in_wav_long'].shape[1] > T > R['mol/in_wav_short'].shape[1] and R['mol/in_wav_eq'].shape[1] == T


def test_mol_parts(R):
    S = int(R['S'])
    te = R['mol/in_te_out_f32'].astype(np.float64)
    d = kl_logistic(te, _in(R, 'mol', 'mean_tot'), _in(R, 'mol', 'scale_tot'), _in(R, 'mol', 'log_scale_tot'),
                    uniforms(R)[0], S)
    assert _close(d['H_bl'], R['mol/parts_H_bl'], 0) < 1e-9
    for k in ('kl_loss', 'H_Ps', 'H_Ps_Pt'):
        assert _close(d[k], R['mol/parts_' + k], 0) < 1e-10, k


def test_mol_full(R):
    S = int(R['S'])
    hp = json.loads(str(R['mol/st_cfg_json']))
    args = (_in(R, 'mol', 'mean_tot'), _in(R, 'mol', 'scale_tot'), _in(R, 'mol', 'log_scale_tot'))
    u_kl, u_cl = uniforms(R)
    te, te_rand = teacher_out(R, 'mol', 'mel'), teacher_out(R, 'mol', 'mel_rand')
    assert np.abs(te.astype(np.float32) - R['mol/in_te_out_f32']).max() <= 1e-6 * max(1.0, np.abs(te).max())
    kl = kl_logistic(te, *args, u_kl, S)
    cl = -kl_logistic(te_rand, *args, u_cl, S)['kl_loss']
    pl = power_loss(_in(R, 'mol', 'x'), _in(R, 'mol', 'wav_long'))
    loss = kl['kl_loss'] + hp['power_loss_factor'] * pl + hp['contrastive_loss_factor'] * cl
    want = {'kl_loss': kl['kl_loss'], 'H_Ps': kl['H_Ps'], 'H_Ps_Pt': kl['H_Ps_Pt'], 'power_loss': pl,
            'contrastive_loss': cl, 'loss': loss}
    # the reference's graph and the oracle compute the teacher in float64 in different orders
    for k, v in want.items():
        assert _close(v, R['mol/full_' + k], 0) < 1e-8, k
    assert _close(kl['H_bl'], R['mol/full_H_bl'], 0) < 1e-7


def test_gauss_parts_and_full(R):
    hp = json.loads(str(R['gauss/st_cfg_json']))
    args = (_in(R, 'gauss', 'mean_tot'), _in(R, 'gauss', 'scale_tot'), _in(R, 'gauss', 'log_scale_tot'))
    d = kl_gauss(R['gauss/in_te_out_f32'].astype(np.float64), *args)
    assert _close(d['kl_bl'], R['gauss/parts_kl_bl'], 0) < 1e-10
    assert _close(d['kl_loss'], R['gauss/parts_kl_loss'], 0) < 1e-10
    f = kl_gauss(teacher_out(R, 'gauss', 'mel'), *args)
    pl = power_loss(_in(R, 'gauss', 'x'), _in(R, 'gauss', 'wav_long'))
    assert _close(f['kl_loss'], R['gauss/full_kl_loss'], 0) < 1e-8
    assert _close(pl, R['gauss/full_power_loss'], 0) < 1e-10
    assert _close(f['kl_loss'] + hp['power_loss_factor'] * pl, R['gauss/full_loss'], 0) < 1e-8
    assert 'gauss/full_contrastive_loss' not in R.files


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
@pytest.mark.parametrize('case', ['eq', 'long', 'short'])
def test_power_loss_trims(R, tag, case):
    pl = power_loss(_in(R, tag, 'x'), _in(R, tag, 'wav_' + case))
    assert _close(pl, R['{}/parts_power_loss_{}'.format(tag, case)], 0) < 1e-10
