"""The layer-group kernel (csrc/wn_iaf_g.hip) issues matrix work and hoisted-tile loads only for the LDS blocks a later
layer, the flow head or the output still reads: per layer the blocks from its `first` on, inside the unit.  A block skipped
by mistake -- or a stale one read where a computed one was due -- shows as a difference between the group form and the
per-layer form, which has no halo and runs on the same engine.

Shapes are chosen for the block pattern of a segment (24 LDS blocks of 16 samples: halo + output blocks, two per wave, wave w
holds blocks w and w + 12), not for size; T = floor(200 F / 512) * 512:

    F = 3   T = 512     natural: 20 + 12 blocks; decimated: ONE active block per residue (only a wave's first block runs)
    F = 6   T = 1 024   natural: a last segment of 4 blocks
    F = 35  T = 6 656   decimated unit of 13 blocks
    F = 80  T = 15 872  decimated unit of 31 blocks: two segments, the second reading halo the first's range produced

each at one and two utterances, on the shipped flows, on [5, 12, 7] (groups with other `first` patterns, two halo blocks)
and on [1].  Unit-gain weights, so that a stale block is not numerically invisible.  Bounds: 4e-6 * max(1, |ref|) between
the forms (the bound of test_gpu_iaf.py::test_layer_groups_match_per_layer_launches: same arithmetic, other summation
partners in the start conv only), bit equality between two runs of the group form."""
import numpy as np
import pytest

from conftest import load_json

pytestmark = pytest.mark.gpu

SHAPES = ((3, 512), (6, 1024), (35, 6656), (80, 15872))
WANT = ('x', 'mean_tot', 'scale_tot')


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('layers', [None, [5, 12, 7], [1]], ids=['shipped', '5-12-7', '1'])
def test_group_form_computes_every_block_a_later_layer_reads(layers):
    from nsynth_wavenet_amd.engine import Engine
    from oracle import wavenet_np as O
    cfgd = load_json('parallel_wavenet.json')
    if layers is not None:
        cfgd = dict(cfgd, num_iaf_layers=layers)
    hp = O.HP(cfgd)
    w = O.synth_weights(hp, 'student', seed=4321, init='unit')
    eng = Engine(cfgd, precision='f16x3').load_weights(w)
    rs = np.random.RandomState(2024)
    try:
        for F, T in SHAPES:
            assert O.iaf_length(F, hp) == T
            for B in (1, 2):
                mel = rs.uniform(0, 1, [B, F, 80]).astype(np.float32)
                noise = O.logistic_from_uniform(rs.uniform(1e-5, 1 - 1e-5, [B, T]))
                eng.set_layer_groups(True)
                assert eng.iaf_layer_groups(B, F)         # ... so that the comparison cannot degenerate into a form against itself
                a = {k: _np(v) for k, v in eng.iaf_generate(mel, noise, want=WANT).items()}
                a2 = {k: _np(v) for k, v in eng.iaf_generate(mel, noise, want=WANT).items()}
                eng.set_layer_groups(False)
                assert not eng.iaf_layer_groups(B, F)
                b = {k: _np(v) for k, v in eng.iaf_generate(mel, noise, want=WANT).items()}
                for k in WANT:
                    assert a[k].shape == b[k].shape and np.isfinite(a[k]).all(), (layers, B, F, k)
                    assert np.array_equal(a[k], a2[k]), (layers, B, F, k)
                    err, bound = np.abs(a[k] - b[k]).max(), 4e-6 * max(1.0, np.abs(b[k]).max())
                    print('layers {} B {} F {} {}: max |group - per-layer| {:.3e} (bound {:.3e})'.format(layers, B, F, k, err, bound))
                    assert err <= bound, (layers, B, F, k)
    finally:
        eng.close()
