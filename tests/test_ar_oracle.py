"""CPU side of the fastgen step tests (tests/test_gpu_ar_heads.py): the references of those tests, held to their own conditions.

1. The K1 bar 2e-5 max(1, max |ref|) is only a test of the kernels if float32 arithmetic itself stays well inside it on the
   cases chosen: on every matrix case of tests/ar_cases.py the float32 oracle step loop (O.Fastgen, the incremental form, fed
   the forced signal) agrees with the float64 full-sequence teacher within HALF the bar, for all 33 utterances a batch of
   the matrix can take and all 80 steps.
2. Every sampler edge row: the "edge is reached" assertions hold on the float64 sampler, and the float32 oracle sampler
   (Fastgen.sample_from) satisfies what the engine is held to (ar_cases.check_edge: parity rule, equality where float32 and
   float64 cannot differ, first index at a tie).
3. The distribution statistics and their 5-standard-error bounds, on the oracle samplers fed numpy draws of the same N, for the
   seed the GPU test uses and ten further ones: the bounds are ones the reference alone stays within.
"""
import numpy as np
import pytest

import ar_cases as A
from oracle import wavenet_np as O


def test_geometries_are_accepted_and_give_the_stated_slabs():
    """wn_host.cpp's width rules (width, skip_width % 64, gate_width % 128, deconv_width % 64) and the batched pack's
    (every K a multiple of 64), restated; K = 3 W + Cd + G/2 as the matrix table states it."""
    for g, d in A.GEOMETRIES.items():
        hp = O.HP(A.config(g, 'mol10'))
        W, S, Cd, G = hp.width, hp.skip_width, hp.deconv_width, O.teacher_gate_width(hp)
        assert W % 64 == 0 and S % 64 == 0 and G % 128 == 0 and Cd % 64 == 0 and (G // 2) % 64 == 0
        assert G == (2 * W if d['double_gate_width'] else W)
        assert 3 * W + Cd + G // 2 == A.SLAB_K[g]
        assert 3 * W + Cd <= 2048 and G // 2 <= 1024                   # the tuned instantiation, not the wide one
    assert A.SLAB_K['A'] % 256 == 0 and A.SLAB_K['B'] % 256 == 64 and A.SLAB_K['C'] % 256 == 128
    rates = [2 ** (i % A.STACK['num_stages']) for i in range(A.STACK['num_layers'])]
    assert rates == [1, 2, 4, 8, 16, 1, 2] and A.TN % 16 == 0 and A.TN >= 2 * (2 * max(rates) + 1)
    heads = {h: [g for g, hh in A.MATRIX if hh == h] for h in A.HEADS}
    assert all(len(v) >= 2 for v in heads.values())
    assert all({'mol10', 'ce', 'gauss'} <= {h for g, h in A.MATRIX if g == geo} for geo in A.GEOMETRIES)
    assert [A.padded_batch(b) for b in A.BATCHES] == [0, 0, 16, 32, 64] and A.padded_batch(A.GEMV_BATCH, gemv=True) == 0
    assert all(A.padded_batch(a) == A.padded_batch(b) for a, b in A.SAME_FORM_PAIRS)
    assert A.padded_batch(4) != A.padded_batch(17)                      # the pair that is NOT asserted bit-equal


@pytest.mark.parametrize('geom,head', A.MATRIX, ids=A.MATRIX_IDS)
def test_float32_oracle_is_inside_half_the_k1_bar(geom, head):
    _, hp, w, enc, forced = A.case(geom, head)
    ref, bar = A.k1_reference(geom, head)
    fg = O.Fastgen(w, hp, A.ROWS, np.float32)
    a = np.zeros([A.ROWS, 1], np.float32)
    err = 0.0
    for t in range(A.TN):
        out = fg.out_params(a, enc[:, t])
        assert out.dtype == np.float32
        err = max(err, float(np.abs(out - ref[:, t]).max()))
        a = forced[:, t:t + 1]
    print('{}-{}: float32 oracle vs float64 teacher: {:.3f} of the K1 bar ({:.3g})'.format(geom, head, err / bar, bar))
    assert err <= 0.5 * bar


def test_forced_signals_keep_clear_of_the_mu_law_steps():
    for geom, head in A.MATRIX:
        _, hp, _, _, forced = A.case(geom, head)
        assert np.abs(forced).max() < 1.0
        if hp.use_mu_law:
            y = np.sign(forced) * np.log1p(255.0 * np.abs(forced.astype(np.float64))) / np.log(256.0) * 128.0
            assert np.abs(y - np.round(y)).min() >= A.MU_LAW_MARGIN
            assert np.array_equal(O.mu_law(forced, dtype=np.float32), O.mu_law(forced, dtype=np.float64))


@pytest.mark.parametrize('loss,i', A.EDGE_IDS)
def test_edge_rows_on_the_float32_oracle(loss, i):
    _, hp, w, _, _ = A.case(A.EDGE_GEOM, A.EDGE_HEADS[loss])
    for B in A.EDGE_BATCHES:
        edges = A.edge_cases(loss, B)
        assert len(edges) == sum(1 for l, _ in A.EDGE_IDS if l == loss)
        edge = edges[i]
        name, row, rnd = edge[:3]
        assert rnd.shape == (A.EDGE_TN, B, A.n_rand(hp)) and rnd.dtype == np.float32
        fg = O.Fastgen(w, hp, B, np.float32)
        out = np.broadcast_to(np.asarray(row, np.float32), (B, A.EDGE_TN, len(row)))
        idx = np.stack([fg.sample_from(out[:, t], rnd[t]) for t in range(A.EDGE_TN)], axis=1)
        A.check_edge('float32 oracle', hp, edge, idx, out)


SEEDS = [A.STAT_SEED] + list(range(1, 11))


@pytest.mark.parametrize('loss', ['gauss', 'mol', 'ce'])
def test_statistics_hold_on_numpy_draws(loss):
    hp = O.HP(A.stat_config(loss))
    row = np.asarray(A.STAT_ROWS[loss], np.float32)
    Q = O.quant_chann_of(hp)
    for seed in SEEDS:
        for B in A.STAT_BATCHES:
            rs = np.random.RandomState(seed)
            N = B * A.STAT_TN
            out = np.broadcast_to(row, (N, row.size))
            if loss == 'gauss':
                idx = O.gauss_sample(out, Q, rs.standard_normal(N), np.float32)
            elif loss == 'mol':
                u = rs.uniform(1e-5, 1 - 1e-5, [N, 4])
                idx = O.mol_sample(out, Q, u[:, :3], u[:, 3], np.float32)
            else:
                idx = O.ce_sample(out, Q, rs.uniform(0, 1, N), np.float32)
            A.assert_statistics('numpy draws, seed {}'.format(seed), loss, idx.reshape(B, A.STAT_TN))


def test_fixed_output_weights_give_the_row_whatever_is_fed_back():
    for loss in ('gauss', 'mol', 'ce'):
        hp = O.HP(A.stat_config(loss))
        w = A.fixed_output_weights(hp, A.STAT_ROWS[loss])
        fg = O.Fastgen(w, hp, 2, np.float32)
        rs = np.random.RandomState(0)
        for t in range(3):
            out = fg.out_params(rs.uniform(-1, 1, [2, 1]), rs.standard_normal([2, hp.deconv_width]))
            assert np.array_equal(out, np.broadcast_to(np.asarray(A.STAT_ROWS[loss], np.float32), out.shape))
