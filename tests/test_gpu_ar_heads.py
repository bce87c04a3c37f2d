"""GPU tests of the fastgen step kernels (csrc/wn_ar.hip) against float64, across output heads, gate widths and batch forms.

Cases, bars and bounds are in tests/ar_cases.py; tests/test_ar_oracle.py (CPU) holds the references to their own conditions.
  1. teacher-forced step outputs (K1) on three geometries x five heads x six batch forms, rows of a batch independent, graph
     replay, and the single-step API with explicit state at B = 5 and 17;
  2. sampler edges on fixed network outputs (out2/W = 0), in the GEMV and the [o][NB] layout;
  3. the distribution of the device-drawn randoms (Philox) on fixed network outputs.
"""
import numpy as np
import pytest

import ar_cases as A

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _rows(x, B):
    """The first B utterances of a case's (shared, read-only) array, as an array of the call's own."""
    return np.array(x[:B])


def _engine(cfgd, w):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(cfgd).load_weights(w)


@pytest.mark.parametrize('geom,head', A.MATRIX, ids=A.MATRIX_IDS)
def test_k1_step_outputs_match_the_float64_teacher(geom, head, monkeypatch):
    """out_params of the teacher-forced step loop against the float64 full-sequence teacher at the bar 2e-5 max(1, max |ref|),
    for B = 1, 3 (GEMV step), 4, 17, 33 (batched step on 16, 32 and 64 columns) and B = 5 on the GEMV step; rows of a batch
    equal the same rows of another batch bit for bit where both run the same step form (ar_cases.SAME_FORM_PAIRS; B = 17
    against B = 4 is across forms and is not asserted); and the sampler parity rule on a free run of each form."""
    from oracle import wavenet_np as O
    monkeypatch.delenv('WN_AR_MODE', raising=False)
    cfgd, hp, w, enc, forced = A.case(geom, head)
    ref, bar = A.k1_reference(geom, head)
    eng = _engine(cfgd, w)
    assert eng.ar_n_rand() == A.n_rand(hp)
    outs = {}
    for B in sorted(set(A.BATCHES) | {b for p in A.SAME_FORM_PAIRS for b in p}):
        o = eng.ar_generate(_rows(enc, B), None, seed=1, forced_wav=_rows(forced, B), want_out=True)
        outs[B] = _np(o['out_params'])
    monkeypatch.setenv('WN_AR_MODE', 'gemv')
    o = eng.ar_generate(_rows(enc, A.GEMV_BATCH), None, seed=1, forced_wav=_rows(forced, A.GEMV_BATCH), want_out=True)
    outs['gemv5'] = _np(o['out_params'])
    monkeypatch.delenv('WN_AR_MODE')
    for key, got in outs.items():
        B = got.shape[0]
        assert got.shape == ref[:B].shape
        err = float(np.abs(got - ref[:B]).max())
        print('K1 {}-{} B={} ({}): max error {:.3f} of the bar'.format(
            geom, head, B, 'GEMV' if key == 'gemv5' or B < 4 else 'NB=%d' % A.padded_batch(B), err / bar))
    for key, got in outs.items():
        B = got.shape[0]
        assert np.abs(got - ref[:B]).max() <= bar, (geom, head, key)
    for a, b in A.SAME_FORM_PAIRS:
        assert np.array_equal(outs[a], outs[b][:a]), (geom, head, a, b)
    assert np.array_equal(outs[3], outs['gemv5'][:3])
    # free run of each form with injected randoms: the sampler on the engine's own outputs, and the fed-back audio
    Q = O.quant_chann_of(hp)
    for B in (3, 17):
        rnd = A.free_run_randoms(hp, A.TN, B, seed=B)
        o = eng.ar_generate(_rows(enc, B), rnd, want_out=True)
        gi = _np(o['idx'])
        assert gi.min() >= -Q // 2 and gi.max() < Q // 2
        A.assert_sampler_parity('free run {}-{} B={}'.format(geom, head, B), hp, _np(o['out_params']), rnd, gi)
        assert np.abs(_np(o['wav']) - A.dequant(gi, hp)).max() <= 2.0 ** -23
    eng.close()


@pytest.mark.parametrize('geom,head', [('B', 'ce'), ('C', 'gauss')])
def test_graph_replay_equals_plain_launches_on_the_batched_step(geom, head):
    import torch
    cfgd, hp, w, enc, forced = A.case(geom, head)
    eng = _engine(cfgd, w)
    B = 17
    rnd = A.free_run_randoms(hp, A.TN, B, seed=3)
    for kw in (dict(forced_wav=_rows(forced, B)), dict()):
        a = eng.ar_generate(_rows(enc, B), rnd, want_out=True, use_graph=True, **kw)
        b = eng.ar_generate(_rows(enc, B), rnd, want_out=True, use_graph=False, **kw)
        for k in ('idx', 'wav', 'out_params'):
            assert torch.equal(a[k], b[k]), (geom, head, k)
    eng.close()


@pytest.mark.parametrize('B', [5, 17])
@pytest.mark.parametrize('geom,head', [('B', 'ce'), ('C', 'gauss')])
def test_single_step_api_with_explicit_state(geom, head, B):
    """40 ar_step calls on ar_new_state(B) (the per_step path of every kernel) against the oracle's step, as test_golden_ar
    does at B <= 3; the indices fed back are the oracle's."""
    from oracle import wavenet_np as O
    cfgd, hp, w, enc, _ = A.case(geom, head)
    eng = _engine(cfgd, w)
    rnd = A.free_run_randoms(hp, 40, B, seed=B + 100)
    encB = _rows(enc, B)
    st = eng.ar_new_state(B)
    fg = O.Fastgen(w, hp, B, np.float32)
    a = np.zeros([B], np.float32)
    worst = 0.0
    outs, idxs = [], []
    for t in range(40):
        s, op = eng.ar_step(st, a, encB[:, t], rnd[t], want_out=True)
        op_o = fg.out_params(a.reshape(B, 1), encB[:, t])
        bar = A.K1_BAR * max(1.0, float(np.abs(op_o).max()))
        err = float(np.abs(_np(op) - op_o).max())
        worst = max(worst, err / bar)
        assert err <= bar, (geom, head, B, t, err / bar)
        outs.append(_np(op))
        idxs.append(_np(s))
        a = fg.dequant(fg.sample_from(op_o, rnd[t])).astype(np.float32)
    print('single-step API {}-{} B={}: max error {:.3f} of the bar'.format(geom, head, B, worst))
    A.assert_sampler_parity('single-step API {}-{} B={}'.format(geom, head, B), hp, np.stack(outs, 1), rnd, np.stack(idxs, 1))
    eng.close()


@pytest.mark.parametrize('loss,i', A.EDGE_IDS)
def test_sampler_edges_on_fixed_outputs(loss, i):
    """One engine whose output is the edge row at every step; the injected randoms sweep against it, at B = 2 (GEMV layout)
    and B = 16 ([o][NB] layout).  ar_cases.check_edge: the edge is reached on the float64 sampler, then the parity rule,
    equality with float64 where float32 cannot differ, the first index at an exact tie, index range, fed-back audio."""
    cfgd, hp, _, enc, _ = A.case(A.EDGE_GEOM, A.EDGE_HEADS[loss])
    eng = None
    for B in A.EDGE_BATCHES:
        edge = A.edge_cases(loss, B)[i]
        if eng is None:
            eng = _engine(cfgd, A.fixed_output_weights(hp, edge[1]))
        o = eng.ar_generate(_rows(enc, B)[:, :A.EDGE_TN], edge[2], want_out=True)
        A.check_edge('engine', hp, edge, _np(o['idx']), _np(o['out_params']), _np(o['wav']))
    eng.close()


@pytest.mark.parametrize('loss', ['gauss', 'mol', 'ce'])
def test_device_drawn_randoms_follow_their_law(loss):
    """rnd=None: Philox draws on the device.  B = 16 (N = 32 768) and B = 2 (N = 4 096) for 2 048 steps on a fixed network
    output; every bound is five standard errors (ar_cases.draw_statistics; held on numpy draws in tests/test_ar_oracle.py)."""
    import torch
    from oracle import wavenet_np as O
    cfgd = A.stat_config(loss)
    hp = O.HP(cfgd)
    row = np.asarray(A.STAT_ROWS[loss], np.float32)
    eng = _engine(cfgd, A.fixed_output_weights(hp, row))
    for B in A.STAT_BATCHES:
        enc = np.zeros([B, A.STAT_TN, hp.deconv_width], np.float32)
        a = eng.ar_generate(enc, None, seed=A.STAT_SEED, want_out=True)
        b = eng.ar_generate(enc, None, seed=A.STAT_SEED)
        c = eng.ar_generate(enc, None, seed=A.STAT_SEED + 1)
        assert torch.equal(a['idx'], b['idx']) and torch.equal(a['wav'], b['wav'])
        assert not torch.equal(a['idx'], c['idx'])
        assert np.array_equal(_np(a['out_params']), np.broadcast_to(row, (B, A.STAT_TN, row.size)))
        gi = _np(a['idx'])
        assert np.abs(_np(a['wav']) - A.dequant(gi, hp)).max() <= 2.0 ** -23
        A.assert_statistics('device draws {} B={}'.format(loss, B), loss, gi)
        A.assert_statistics('device draws {} B={} seed+1'.format(loss, B), loss, _np(c['idx']))
    eng.close()
