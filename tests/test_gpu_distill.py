"""GPU tests of the distillation losses (csrc/wn_distill.hip; ParallelWavenet.kl_loss_logistic / kl_loss_gauss / power_loss /
contrastive_loss / calculate_loss, wavenet/parallel_wavenet.py:361-512) against tests/golden/ref_distill.npz -- what the
reference's own code computed (tests/golden/make_ref_distill.py) -- and against float64 torch compositions of its formulas."""
import json
import os
import threading

import numpy as np
import pytest

from conftest import load_json

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')


@pytest.fixture(scope='module')
def R():
    return np.load(GOLD)


def _np(t):
    return t.detach().cpu().numpy()


def _teacher(cfgd, seed=1234, init='unit'):
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    return Wavenet(cfgd).load_weights(O.synth_weights(O.HP(cfgd), 'teacher', seed=seed, init=init))


@pytest.fixture(scope='module')
def teachers(R):
    return {tag: _teacher(json.loads(str(R[tag + '/te_cfg_json'])), int(R[tag + '/te_seed']), str(R[tag + '/te_init']))
            for tag in ('mol', 'gauss')}


def _in(R, tag, k):
    return R['{}/in_{}'.format(tag, k)]


def _rl(R, key):
    """the reference's logistic draws log u - log(1 - u) of its [B*S, T] uniforms, as [B, S, T] (utils.tf_repeat order);
    the uniforms are regenerated from the golden's seed (tests/golden/make_ref_distill.uniforms)"""
    B, T = R['mol/in_x'].shape
    S = int(R['S'])
    u = np.random.RandomState(int(R['mol/u_seed'])).uniform(1e-5, 1 - 1e-5, [2, B * S, T]).astype(np.float32)
    u = u[{'u_kl': 0, 'u_cl': 1}[key]].astype(np.float64)
    return (np.log(u) - np.log(1.0 - u)).astype(np.float32).reshape(B, S, T)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(1.0, abs(float(b)))


def _per_sample_ok(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def test_mol_xent_kernel_matches_reference(R, teachers):
    eng = teachers['mol'].engine
    S = int(R['S'])
    r = eng.distill_mol_xent(_in(R, 'mol', 'te_out_f32'), _in(R, 'mol', 'mean_tot'), _in(R, 'mol', 'scale_tot'), S,
                             noise=_rl(R, 'u_kl'))
    hb = _np(r['H_bl'])
    assert _per_sample_ok(hb, R['mol/parts_H_bl']) <= 2e-5
    s = _np(r['sums'])
    n = hb.size
    assert _rel(s[0] / n, R['mol/parts_H_Ps_Pt']) <= 1e-5
    assert _rel(s[1] / n + 2, R['mol/parts_H_Ps']) <= 1e-5
    assert _rel(s[0] / n - (s[1] / n + 2), R['mol/parts_kl_loss']) <= 1e-5
    assert abs(s[0] - hb.astype(np.float64).sum()) <= 1e-6 * max(1.0, abs(s[0]))


def test_gauss_kl_kernel_matches_reference(R, teachers):
    eng = teachers['gauss'].engine
    r = eng.distill_gauss_kl(_in(R, 'gauss', 'te_out_f32'), _in(R, 'gauss', 'mean_tot'), _in(R, 'gauss', 'scale_tot'))
    kb = _np(r['kl_bl'])
    assert _per_sample_ok(kb, R['gauss/parts_kl_bl']) <= 2e-5
    s = _np(r['sums'])
    assert _rel(s[0] / kb.size + 4.0 * s[1] / kb.size, R['gauss/parts_kl_loss']) <= 1e-5


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
@pytest.mark.parametrize('case', ['eq', 'long', 'short'])
def test_power_loss_matches_reference(R, tag, case):
    from nsynth_wavenet_amd.engine import power_loss
    x, wav = _in(R, tag, 'x'), _in(R, tag, 'wav_' + case)
    got = float(power_loss(x, wav, device='cuda:0'))
    assert _rel(got, R['{}/parts_power_loss_{}'.format(tag, case)]) <= 1e-5, (got, float(R['{}/parts_power_loss_{}'.format(tag, case)]))
    # and with the roles swapped (the other signal trimmed)
    got2 = float(power_loss(wav, x, device='cuda:0'))
    assert _rel(got2, got) <= 1e-5


def _ff_dict(R, tag):
    import torch
    d = {k: torch.as_tensor(_in(R, tag, k)).cuda() for k in ('mel', 'mel_rand', 'x', 'mean_tot', 'scale_tot', 'log_scale_tot')}
    d['wav'] = torch.as_tensor(_in(R, tag, 'wav_long')).cuda()
    return d


@pytest.mark.parametrize('tag', ['mol', 'gauss'])
def test_calculate_loss_end_to_end(R, teachers, tag):
    """ParallelWavenet(hp, teacher=Wavenet(te_hp)).calculate_loss: the teacher's forward on the unclipped x, the loss kernels,
    the reference's hparams reads and dict."""
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    hp = json.loads(str(R[tag + '/st_cfg_json']))
    pw = ParallelWavenet(hp, teacher=teachers[tag])
    kw = {'noise': _rl(R, 'u_kl'), 'cl_noise': _rl(R, 'u_cl')} if tag == 'mol' else {}
    got = pw.calculate_loss(_ff_dict(R, tag), **kw)
    want = [k[len(tag) + 6:] for k in R.files if k.startswith(tag + '/full_') and R[k].ndim == 0]
    assert sorted(got) == sorted(want)
    for k in want:
        assert _rel(got[k], R['{}/full_{}'.format(tag, k)]) <= 1e-5, (k, float(got[k]), float(R['{}/full_{}'.format(tag, k)]))
    pw.engine.close()


def test_teacher_scores_unclipped_samples(R, teachers):
    """Without mu-law the teacher's input copies samples outside [-1, 1] unclamped (tg_input_kernel), as the reference's
    wav_scaled path does (CLIP = False): the forward on x differs from the forward on clip(x)."""
    x = _in(R, 'mol', 'x')
    assert np.abs(x).max() > 1.0
    eng = teachers['mol'].engine
    a = _np(eng.teacher_forward(x, _in(R, 'mol', 'mel')))
    b = _np(eng.teacher_forward(np.clip(x, -1, 1), _in(R, 'mol', 'mel')))
    assert np.abs(a - b).max() > 1e-3
    ref = R['mol/in_te_out_f32']                  # the reference's teacher output, rounded to float32
    assert np.abs(a - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


def test_device_noise(R, teachers):
    import torch
    eng = teachers['mol'].engine
    te, mean, scale = (torch.as_tensor(_in(R, 'mol', k)).cuda() for k in ('te_out_f32', 'mean_tot', 'scale_tot'))
    S = 8
    r1 = eng.distill_mol_xent(te, mean, scale, S, seed=7, want_noise=True)
    r2 = eng.distill_mol_xent(te, mean, scale, S, noise=r1['noise'])
    r3 = eng.distill_mol_xent(te, mean, scale, S, seed=7, want_noise=True)
    r4 = eng.distill_mol_xent(te, mean, scale, S, seed=8, want_noise=True)
    assert torch.equal(r1['H_bl'], r2['H_bl']) and torch.equal(r1['sums'], r2['sums'])
    assert torch.equal(r1['H_bl'], r3['H_bl']) and torch.equal(r1['noise'], r3['noise']) and torch.equal(r1['sums'], r3['sums'])
    assert float((r1['noise'] == r4['noise']).float().mean()) < 1e-3
    nz = _np(r1['noise'])
    assert 0.9 < nz.std() / (np.pi / np.sqrt(3.0)) < 1.1 and abs(nz.mean()) < 0.05      # logistic(0, 1)


def test_device_noise_agrees_with_injected_at_large_S(R, teachers):
    """Two independent estimates at S = 256 -- device draws and injected numpy draws -- agree within 5 sigma of their own
    per-row spread: the spread of -log p over each estimate's draws, every draw scored on its own (S = 1 calls on the draws
    the calls used), fixed seeds."""
    import torch
    eng = teachers['mol'].engine
    te, mean, scale = (torch.as_tensor(_in(R, 'mol', k)).cuda() for k in ('te_out_f32', 'mean_tot', 'scale_tot'))
    B, T = mean.shape
    S = 256
    u = np.random.RandomState(77).uniform(1e-5, 1 - 1e-5, [B, S, T])
    noise_inj = torch.as_tensor((np.log(u) - np.log(1 - u)).astype(np.float32)).cuda()
    inj = eng.distill_mol_xent(te, mean, scale, S, noise=noise_inj)['H_bl']
    dv = eng.distill_mol_xent(te, mean, scale, S, seed=1001, want_noise=True)

    def per_draw(noise):
        return torch.stack([eng.distill_mol_xent(te, mean, scale, 1, noise=noise[:, s:s + 1].contiguous())['H_bl']
                            for s in range(S)], dim=1).double()           # [B,S,T]: -log p of every draw
    pi, pd = per_draw(noise_inj), per_draw(dv['noise'])
    assert float((pi.mean(dim=1) - inj.double()).abs().max()) <= 1e-4 * max(1.0, float(inj.abs().max()))
    sigma = torch.sqrt(pi.var(dim=1) / S + pd.var(dim=1) / S) + 1e-6
    diff = (dv['H_bl'] - inj).double()
    z_rows = _np(diff.abs() / sigma)
    assert np.mean(z_rows > 5.0) < 1e-2, float(np.mean(z_rows > 5.0))
    z_all = abs(float(diff.sum())) / float(torch.sqrt((sigma ** 2).sum()))
    assert z_all < 5.0, z_all


def test_full_size_mol_xent():
    """parallel_wavenet.json's shape with wavenet_mol.json: B = 1, F = 384, T = 76 800, S = 100.  The fused kernel against a
    float64 torch composition of mol_log_probs on the same out_params (in slices), and its memory: nothing of [B,S,T,.]."""
    import torch
    te_cfg = load_json('wavenet_mol.json')
    teacher = _teacher(te_cfg, seed=1234, init='tf')
    eng = teacher.engine
    B, F, T, S = 1, 384, 76800, 100
    rs = np.random.RandomState(5)
    mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
    x = np.clip(0.2 * rs.standard_normal([B, T]), -1.2, 1.2).astype(np.float32)
    out = eng.teacher_forward(x, mel)
    mean = torch.as_tensor(x + 0.01 * rs.standard_normal([B, T]).astype(np.float32)).cuda()
    scale = torch.as_tensor(np.exp(rs.uniform(-7, -2, [B, T])).astype(np.float32)).cuda()
    eng.distill_mol_xent(out, mean, scale, S, seed=3)              # workspace in place
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = eng.distill_mol_xent(out, mean, scale, S, seed=3)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base - (r['H_bl'].numel() * 4 + r['sums'].numel() * 8)
    assert grown < 64 * 2 ** 20, grown
    rn = eng.distill_mol_xent(out, mean, scale, S, seed=3, want_noise=True)
    assert torch.equal(rn['H_bl'], r['H_bl'])
    noise = rn['noise'].double()
    M = te_cfg['mol_mix']
    Q = 65536.0
    ref = torch.empty(B, T, dtype=torch.float64, device=out.device)
    for t0 in range(0, T, 4096):
        t1 = min(T, t0 + 4096)
        p = out[:, t0:t1].double()                                  # [B,t,3M]
        lg, mu, ls = p[..., :M], p[..., M:2 * M], torch.clamp(p[..., 2 * M:], min=-7.0)
        inv = torch.exp(-ls)
        xx = noise[:, :, t0:t1] * scale[:, None, t0:t1].double() + mean[:, None, t0:t1].double()     # [B,S,t]
        c = xx[..., None] - mu[:, None]
        plus, mn = inv[:, None] * (c + 1.0 / Q), inv[:, None] * (c - 1.0 / Q)
        delta = torch.sigmoid(plus) - torch.sigmoid(mn)
        max_thres, min_thres = (Q - 1 - 0.5) / (Q / 2) - 1.0, 0.5 / (Q / 2) - 1.0
        xe = xx[..., None].expand_as(plus)
        lp = torch.where(xe < min_thres, plus - torch.nn.functional.softplus(plus),
                         torch.where(xe > max_thres, -torch.nn.functional.softplus(mn),
                                     torch.log(torch.clamp(delta, min=1e-12))))
        lp = lp + torch.log_softmax(lg, dim=-1)[:, None]
        ref[:, t0:t1] = -torch.logsumexp(lp, dim=-1).mean(dim=1)
    ref = _np(ref)
    got = _np(r['H_bl'])
    assert _per_sample_ok(got, ref) <= 2e-5
    assert _rel(float(r['sums'][0]) / T, ref.mean()) <= 1e-5
    teacher.engine.close()


def _expect_refusal(fn, text):
    with pytest.raises((ValueError, RuntimeError)) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_invalid_calls_are_refused(R, teachers, student_cfg):
    import torch
    from nsynth_wavenet_amd.engine import Engine
    te = torch.as_tensor(_in(R, 'mol', 'te_out_f32')).cuda()
    mean, scale = (torch.as_tensor(_in(R, 'mol', k)).cuda() for k in ('mean_tot', 'scale_tot'))
    g = torch.as_tensor(_in(R, 'gauss', 'te_out_f32')).cuda()
    mol, gauss = teachers['mol'].engine, teachers['gauss'].engine
    _expect_refusal(lambda: mol.distill_mol_xent(te, mean, scale, 0), 'num_samples')
    _expect_refusal(lambda: mol.distill_mol_xent(te[..., :27].contiguous(), mean, scale, 4), 'out_width')
    _expect_refusal(lambda: gauss.distill_mol_xent(g, mean, scale, 4), 'loss_type is not mol')
    _expect_refusal(lambda: mol.distill_gauss_kl(te, mean, scale), 'loss_type is not gauss')
    st = Engine(student_cfg)
    _expect_refusal(lambda: st.distill_mol_xent(te, mean, scale, 4), 'student handle')
    _expect_refusal(lambda: st.distill_gauss_kl(g, mean, scale), 'student handle')
    st.close()
    ce_cfg = json.loads(str(np.load(os.path.join(os.path.dirname(GOLD), 'ar_ce_mulaw.npz'))['cfg_json']))
    ce = Engine(ce_cfg)
    _expect_refusal(lambda: ce.distill_mol_xent(te, mean, scale, 4), 'cross-entropy')
    ce.close()
    mu_cfg = dict(json.loads(str(R['mol/te_cfg_json'])), use_mu_law=True)
    mu = Engine(mu_cfg)
    _expect_refusal(lambda: mu.distill_mol_xent(te, mean, scale, 4), 'mu-law')
    mu.close()
    # the mirror refuses what the reference asserts (parallel_wavenet.py:133-135) and a call without a teacher
    from nsynth_wavenet_amd.wavenet.parallel_wavenet import ParallelWavenet
    pw = ParallelWavenet(json.loads(str(R['mol/st_cfg_json'])), teacher=teachers['gauss'])
    _expect_refusal(lambda: pw.kl_loss_logistic(_ff_dict(R, 'mol'), 4), 'pairs logistic with mol')
    pw.engine.close()
    pw = ParallelWavenet(json.loads(str(R['mol/st_cfg_json'])))
    _expect_refusal(lambda: pw.kl_loss_logistic(_ff_dict(R, 'mol'), 4), 'needs the teacher')
    pw.engine.close()


def test_two_threads_on_one_teacher_handle(R, teachers):
    """WORK-call contract (include/wnhip.h): two host threads, one handle, own streams and workspaces -- results
    bit-identical to serial runs."""
    import torch
    eng = teachers['mol'].engine
    te, mean, scale = (torch.as_tensor(_in(R, 'mol', k)).cuda() for k in ('te_out_f32', 'mean_tot', 'scale_tot'))
    serial = {s: eng.distill_mol_xent(te, mean, scale, 32, seed=s) for s in (11, 12)}
    torch.cuda.synchronize()
    got, errs = {}, []

    def work(seed):
        try:
            f = eng.fork()
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                rs = [f.distill_mol_xent(te, mean, scale, 32, seed=seed) for _ in range(8)]
            st.synchronize()
            got[seed] = rs
        except Exception as e:                                     # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(s,)) for s in (11, 12)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for s in (11, 12):
        for r in got[s]:
            assert torch.equal(r['H_bl'], serial[s]['H_bl']) and torch.equal(r['sums'], serial[s]['sums'])
