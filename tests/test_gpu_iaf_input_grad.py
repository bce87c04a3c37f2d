"""wn_iaf_backward_input (csrc/wn_iaf_train.hip) behind Engine.iaf_backward_input: d noise of the student against
input_grad_oracle64.student_input_grads in float64 (held to central differences by tests/test_input_grad_oracle.py), at the
project's bar max |g - g64| <= TOL max |g64| (TOL of tests/test_gpu_distill_grad.py, imported); d_encoding is held to
iaf_backward_weights' bits, which tests/test_gpu_student_grad.py holds to the oracle.

Models S1 and S2 of tests/student_grad_oracle64.py with the B / F / T and seed of tests/test_gpu_student_grad.py, chosen there
for near_tie_fraction <= 1e-4 and clamps_inactive -- both re-asserted here.  T = 200 and 264 are no multiples of 256."""
import numpy as np
import pytest

import input_grad_cases as C
import input_grad_oracle64 as IG
import student_grad_oracle64 as S
from test_gpu_distill_grad import TOL

pytestmark = pytest.mark.gpu

_ENG, _ORA = {}, {}


def _np(t):
    return t.detach().cpu().numpy()


def _new_engine(model, seed=C.IAF_SEED):
    from nsynth_wavenet_amd.engine import Engine
    return Engine(C.IAF_CFG[model], kind='student').load_weights(C.iaf_weights(model, seed)[1])


def _engine(model):
    if model not in _ENG:
        _ENG[model] = _new_engine(model)
    return _ENG[model]


def _oracle(tag):
    """(oracle, mel, noise, dense cotangents, the float64 input gradients, StudentGrad64.grads' aux), computed once"""
    if tag not in _ORA:
        hp, w = C.iaf_weights(C.IAF_CASES[tag][0])
        mel, noise, cot = C.iaf_inputs(tag)
        ora = S.StudentGrad64(w, hp)
        _ORA[tag] = (ora, mel, noise, cot, IG.student_input_grads(ora, mel, noise, cot), ora.grads(mel, noise, *cot)['aux'])
    return _ORA[tag]


def _err(label, got, ref):
    g = _np(got).astype(np.float64)
    assert g.shape == ref.shape and np.isfinite(g).all(), label
    e = np.abs(g - ref).max() / np.abs(ref).max()
    print('{} max |g - g64| / max |g64| = {:.2e} (max |g64| {:.3e})'.format(label, e, np.abs(ref).max()))
    return e


@pytest.mark.parametrize('tag', sorted(C.IAF_CASES))
def test_d_noise_matches_the_oracle(tag):
    """dense cotangents: d noise, every element; the last three samples of every row, where the start conv transposed has
    fewer taps, on their own; d_encoding bit-equal to iaf_backward_weights' on the same tape and cotangents"""
    import torch
    model, (B, F, T) = C.IAF_CASES[tag]
    ora, mel, noise, cot, ref, aux = _oracle(tag)
    assert S.near_tie_fraction(aux) <= 1e-4
    assert S.clamps_inactive(aux)
    eng = _engine(model)
    assert eng.iaf_length(F) == T
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    res = eng.iaf_backward_input(tape, *cot)
    assert tuple(res['d_noise'].shape) == (B, T)
    e = _err('IAF-IN {} d_noise'.format(tag), res['d_noise'], ref['d_noise'])
    tail = np.abs(_np(res['d_noise']).astype(np.float64)[:, -3:] - ref['d_noise'][:, -3:]).max() / np.abs(ref['d_noise']).max()
    print('IAF-IN {} d_noise, last three samples of each row: {:.2e} of max |g64|; their own max {:.3e}'.format(
        tag, tail, np.abs(ref['d_noise'][:, -3:]).max()))
    assert np.abs(ref['d_noise'][:, -3:]).min() > 0
    ed = max(np.abs(_np(res['d_encoding'][s]).astype(np.float64) - ref['d_encoding'][s]).max() / np.abs(ref['d_encoding'][s]).max()
             for s in range(ref['d_encoding'].shape[0]))
    print('IAF-IN {} d_encoding {:.2e}'.format(tag, ed))
    wres = eng.iaf_backward_weights(tape, *cot)
    assert torch.equal(res['d_encoding'].view(torch.int32), wres['d_encoding'].view(torch.int32))
    again = eng.iaf_backward_input(tape, *cot, want_encoding=False)
    assert again['d_encoding'] is None
    assert torch.equal(again['d_noise'].view(torch.int32), res['d_noise'].view(torch.int32)), 'repeat, without d_encoding'
    assert e <= TOL and tail <= TOL and ed <= TOL, (tag, e, tail, ed)


def test_single_cotangents_at_the_row_ends():
    """S1a: one non-zero cotangent sample at t0 = T - 1, T - 2, T - 3 and 0 of row 0, against the oracle"""
    model, (B, F, T) = C.IAF_CASES['S1a']
    ora, mel, noise, _, _, _ = _oracle('S1a')
    eng = _engine(model)
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    for t0 in (T - 1, T - 2, T - 3, 0):
        cot = [np.zeros((B, T), np.float32) for _ in range(3)]
        for i, v in enumerate((0.75, -1.5, 2.0)):
            cot[i][0, t0] = v
        ref = IG.student_input_grads(ora, mel, noise, cot)['d_noise']
        e = _err('IAF-IN S1a single t0 = {}'.format(t0), eng.iaf_backward_input(tape, *cot, want_encoding=False)['d_noise'], ref)
        assert e <= TOL, (t0, e)


@pytest.mark.parametrize('tag', ['S1b', 'S2'])
def test_d_noise_is_causal_and_rows_are_independent(tag):
    """cotangents non-zero at one t0 only: d_noise[t > t0] == 0 exactly; cotangents that are zero in batch row 0: d_noise row 0
    is exactly zero"""
    import torch
    model, (B, F, T) = C.IAF_CASES[tag]
    ora, mel, noise, cot, _, _ = _oracle(tag)
    eng = _engine(model)
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    for t0 in (0, T // 2 + 1, T - 2):
        one = [np.zeros_like(c) for c in cot]
        for o, c in zip(one, cot):
            o[:, t0] = c[:, t0]
        d = _np(eng.iaf_backward_input(tape, *one, want_encoding=False)['d_noise'])
        assert np.all(d[:, t0 + 1:] == 0), (t0, 'the future leaks into d_noise')
        assert np.all(d[:, t0] != 0), t0
    if B > 1:
        zero0 = [c.copy() for c in cot]
        for c in zero0:
            c[0] = 0
        d = eng.iaf_backward_input(tape, *zero0)
        assert int((d['d_noise'][0].view(torch.int32) & 0x7fffffff != 0).sum()) == 0
        assert float(d['d_noise'][1:].abs().max()) > 0
        assert int((d['d_encoding'][:, 0].contiguous().view(torch.int32) & 0x7fffffff != 0).sum()) == 0


def test_refusals():
    """by message: a teacher handle, a tape of another handle, a wrong B / F / T, a copied tape; the size query returns 0 for
    a handle the call refuses"""
    import os
    import distill_oracle64 as D
    from oracle import wavenet_np as O
    from nsynth_wavenet_amd.wavenet.wavenet import Wavenet
    import torch
    B, F, T = C.IAF_CASES['S1a'][1]
    mel, noise, cot = C.iaf_inputs('S1a')
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_distill.npz')
    te_cfg, te_seed, te_init = D.golden_case(np.load(gold), 'mol')[1]
    te = Wavenet(te_cfg).load_weights(O.synth_weights(O.HP(te_cfg), 'teacher', seed=te_seed, init=te_init))
    try:
        assert int(te.engine.lib.wn_iaf_backward_input_workspace_bytes(te.engine._h, B, F, T)) == 0
        with pytest.raises(ValueError, match='wn_iaf_backward_input: handle is not a ParallelWavenet student'):
            te.engine.iaf_backward_input(torch.zeros(4096, dtype=torch.uint8, device='cuda'), *cot, n_frames=F)
    finally:
        te.engine.close()
    eng = _engine('S1')
    assert int(eng.lib.wn_iaf_backward_input_workspace_bytes(eng._h, B, F, T)) > 0
    assert int(eng.lib.wn_iaf_backward_input_workspace_bytes(eng._h, B, F, T)) < \
        int(eng.lib.wn_iaf_backward_weights_workspace_bytes(eng._h, B, F, T))
    assert int(eng.lib.wn_iaf_backward_input_workspace_bytes(eng._h, B, F, T - 1)) == 0
    _, tape = eng.iaf_forward_train_tape(mel, noise=noise)
    with pytest.raises(ValueError, match='wn_iaf_backward_input: the tape was not written by wn_iaf_forward_train_tape of this handle'):
        eng.iaf_backward_input(tape.clone(), *cot, n_frames=F)
    other = _new_engine('S1', seed=C.IAF_SEED + 1)
    try:
        with pytest.raises(ValueError, match='was not written by wn_iaf_forward_train_tape of this handle'):
            other.iaf_backward_input(tape, *cot, n_frames=F)
        # an engine object that wrote no tape knows no frame count (it keeps them by address, and in `eng` a copy may land
        # on the address of an earlier, freed tape)
        with pytest.raises(ValueError, match='pass n_frames'):
            other.iaf_backward_input(tape, *cot)
    finally:
        other.close()
    with pytest.raises(ValueError, match='the tape holds B = 2, T = 200, not B = 1, T = 200'):
        eng.iaf_backward_input(tape, *[c[:1] for c in cot], n_frames=F)
    with pytest.raises(ValueError, match='the tape holds F = 25 mel frames, not 26'):
        eng.iaf_backward_input(tape, *cot, n_frames=F + 1)
    with pytest.raises(ValueError, match='not a multiple of the largest dilation'):
        eng.iaf_backward_input(tape, *[c[:, :T - 1] for c in cot], n_frames=F)
    with pytest.raises(ValueError, match='the tape holds B = 2, T = 200, not B = 2, T = 196'):
        eng.iaf_backward_input(tape, *[c[:, :T - 4] for c in cot], n_frames=F)
    eng.iaf_backward_input(tape, *cot)              # and the tape is still good
    torch.cuda.synchronize()


def teardown_module(module):
    for e in _ENG.values():
        e.close()
    _ENG.clear()
