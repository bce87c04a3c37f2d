"""GPU tests of the device-resident dataset and its batch kernel (wn_train_batch, csrc/wn_batch.hip) behind
train.DeviceDataset.  Crop lengths: 1200 (7 frames, one partial workgroup), 1600 (9 frames: the second workgroup holds one
frame) and 7680 (39 frames, the shipped wave_length); B in {1, 3, 8}; a pool of six noise utterances whose lengths include
exactly L, L + 1 and three shorter than L.

Everything but one bar is bit equality: the picks against the numpy twin train.batch_picks, wav against the pool slices, mel
and mel_rand against wn_mel_spectrogram (mel_extractor.batch_melspectrogram_device) of the materialised crops.  The one bar,
2e-5 against the host featuriser on the host route's batch, is the agreement tests/test_mel.py asks of two featurisers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LENGTHS = [1200, 1600, 7680]
BATCHES = [1, 3, 8]
SEED = 5


def _pool(L, seed=0):
    rs = np.random.RandomState(seed + L)
    lengths = [L - 1, L, 700, L + 1, 3 * L + 17, 1025]
    return [rs.uniform(-0.5, 0.5, n).astype(np.float32) for n in lengths]


_DS, _OUT = {}, {}


def _dataset(L):
    from nsynth_wavenet_amd import train
    if L not in _DS:
        _DS[L] = train.DeviceDataset(_pool(L), L, seed=SEED)
    return _DS[L]


def _batch(L, B):
    """the batch of step 11 with mel_rand, computed once per shape and left unchanged"""
    if (L, B) not in _OUT:
        _OUT[L, B] = _dataset(L).batch(11, B, mel_rand=True)
    return _OUT[L, B]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _crops(ds, picks):
    return np.stack([ds.utterances[u][t:t + ds.length] for u, t in picks])


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('L', LENGTHS)
def test_picks_equal_the_numpy_twin(L, B):
    import torch
    from nsynth_wavenet_amd import train
    ds, out = _dataset(L), _batch(L, B)
    assert out['picks'].dtype == torch.int64 and tuple(out['picks'].shape) == (2, B, 2)
    for s in (0, 1):
        want = train.batch_picks(SEED, 11, B, ds.lengths, L, stream=s)
        assert np.array_equal(_np(out['picks'][s]), want), (s, _np(out['picks'][s]), want)
    # only the three utterances of at least L samples are picked
    assert set(_np(out['picks'])[..., 0].ravel().tolist()) <= {1, 3, 4}


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('L', LENGTHS)
def test_wav_is_the_pool_slice(L, B):
    import torch
    ds, out = _dataset(L), _batch(L, B)
    assert tuple(out['wav'].shape) == (B, L) and out['wav'].dtype == torch.float32
    want = _crops(ds, _np(out['picks'][0]))
    assert np.array_equal(_np(_bits(out['wav'])), want.view(np.int32))


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('L', LENGTHS)
def test_mel_is_the_featuriser_of_the_crop(L, B):
    """bit for bit against wn_mel_spectrogram of the materialised crops, both streams; 2e-5 against the host route"""
    from nsynth_wavenet_amd.auxilaries import mel_extractor as M
    ds, out = _dataset(L), _batch(L, B)
    F = 1 + L // 200
    assert tuple(out['mel'].shape) == tuple(out['mel_rand'].shape) == (B, F, 80)
    for s, key in enumerate(('mel', 'mel_rand')):
        crops = _crops(ds, _np(out['picks'][s]))
        want = M.batch_melspectrogram_device(crops)
        d = int((_bits(out[key]).long() - _bits(want).long()).abs().max())
        print('{} L {} B {}: largest difference of the bit patterns {}'.format(key, L, B, d))
        assert d == 0
    host = ds.host_batch(11, B, mel_rand=True)
    assert np.array_equal(host['picks'], _np(out['picks'])) and np.array_equal(host['wav'].view(np.int32), _np(_bits(out['wav'])))
    for key in ('mel', 'mel_rand'):
        err = float(np.abs(_np(out[key]).astype(np.float64) - host[key]).max())
        print('{} L {} B {}: largest difference from the host featuriser {:.3g}'.format(key, L, B, err))
        assert err <= 2e-5


def _contained(L, order):
    """the batch of a pool in which only the utterance of exactly L samples is eligible, its neighbours filled with `fill`"""
    from nsynth_wavenet_amd import train
    rs = np.random.RandomState(L)
    core = rs.uniform(-0.5, 0.5, L).astype(np.float32)
    outs = []
    for fill in (np.nan, 0.0):
        utts = [core if k == 'E' else np.full(k, fill, np.float32) for k in order]
        ds = train.DeviceDataset(utts, L, seed=1)
        outs.append(ds.batch(3, 3, mel_rand=True))
    return core, order.index('E'), outs


@pytest.mark.parametrize('order', [(1100, 'E', 900), ('E', 1100), (1100, 'E')], ids=['between', 'first', 'last'])
@pytest.mark.parametrize('L', LENGTHS)
def test_no_load_leaves_the_crop(L, order):
    """NaN on both sides of an utterance of exactly L samples (every start is 0, the crop is the whole utterance): every
    output is finite and the bits of the run with those neighbours zeroed"""
    import torch
    core, at, (a, b) = _contained(L, order)
    assert np.array_equal(_np(a['picks']), np.tile(np.array([at, 0], np.int64), (2, 3, 1)))
    for key in ('wav', 'mel', 'mel_rand'):
        assert bool(torch.isfinite(a[key]).all()), key
        assert torch.equal(_bits(a[key]), _bits(b[key])), key
    assert np.array_equal(_np(a['wav'][2]), core)
    assert torch.equal(a['mel'], a['mel_rand'])                      # both streams featurise the same crop here


def _raw_call(ds, B, ns, fill, step=11):
    """wn_train_batch on output buffers pre-filled with `fill` bytes"""
    import torch
    L, F = ds.length, ds.frames
    wav = torch.full((B, L), fill, dtype=torch.float32, device='cuda')
    mel = torch.full((ns, B, F, 80), fill, dtype=torch.float32, device='cuda')
    picks = torch.full((ns, B, 2), -7, dtype=torch.int64, device='cuda')
    rc = ds.lib.wn_train_batch(ds.pool.data_ptr(), ds.utt_off.data_ptr(), ds.utt_len.data_ptr(), ds.eligible.data_ptr(),
                               int(ds.eligible.numel()), B, L, ds.seed, step, ns, wav.data_ptr(), mel.data_ptr(), picks.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ds.lib.wn_last_error(None)
    return wav, mel, picks


@pytest.mark.parametrize('L', LENGTHS)
def test_outputs_do_not_depend_on_the_buffers_or_on_n_streams(L):
    """buffers pre-filled with NaN; n_streams = 1 writes no second stream and gives stream 0's bits"""
    import torch
    B = 3
    ds, out = _dataset(L), _batch(L, B)
    wav, mel, picks = _raw_call(ds, B, 2, float('nan'))
    assert torch.equal(_bits(wav), _bits(out['wav'])) and torch.equal(picks, out['picks'])
    assert torch.equal(_bits(mel[0]), _bits(out['mel'])) and torch.equal(_bits(mel[1]), _bits(out['mel_rand']))
    wav1, mel1, picks1 = _raw_call(ds, B, 1, float('nan'))
    assert torch.equal(_bits(wav1), _bits(out['wav'])) and torch.equal(_bits(mel1[0]), _bits(out['mel']))
    assert torch.equal(picks1[0], out['picks'][0])
    single = ds.batch(11, B)
    assert sorted(single) == ['mel', 'picks', 'wav'] and tuple(single['picks'].shape) == (1, B, 2)
    assert torch.equal(_bits(single['mel']), _bits(out['mel'])) and torch.equal(_bits(single['wav']), _bits(out['wav']))
    # another step is another batch; the same step is the same batch
    assert not torch.equal(ds.batch(12, B)['picks'], single['picks']) and torch.equal(ds.batch(11, B)['picks'], single['picks'])


def test_refusals():
    import torch
    from nsynth_wavenet_amd import train
    ds = _dataset(1200)
    lib, B, L = ds.lib, 2, 1200
    wav = torch.zeros(B, L, device='cuda')
    mel = torch.zeros(2, B, 7, 80, device='cuda')
    picks = torch.zeros(2, B, 2, dtype=torch.int64, device='cuda')
    good = dict(pool=ds.pool.data_ptr(), off=ds.utt_off.data_ptr(), len=ds.utt_len.data_ptr(), el=ds.eligible.data_ptr(),
                n=int(ds.eligible.numel()), B=B, L=L, ns=2, wav=wav.data_ptr(), mel=mel.data_ptr(), picks=picks.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.wn_train_batch(a['pool'], a['off'], a['len'], a['el'], a['n'], a['B'], a['L'], 0, 0, a['ns'], a['wav'], a['mel'],
                                a['picks'], None)
        return rc, (lib.wn_last_error(None) or b'').decode()

    for key in ('pool', 'off', 'len', 'el', 'wav', 'mel', 'picks'):
        rc, msg = call(**{key: None})
        assert rc == -22 and 'wn_train_batch: null pointer' in msg, (key, rc, msg)
    for kw, text in (({'B': 0}, 'B must be >= 1'), ({'L': 1024}, 'need more than 1024'), ({'L': 0}, 'need more than 1024'),
                     ({'n': 0}, 'n_eligible must be >= 1'), ({'ns': 0}, 'n_streams must be 1 or 2'),
                     ({'ns': 3}, 'n_streams must be 1 or 2')):
        rc, msg = call(**kw)
        assert rc == -22 and msg.startswith('wn_train_batch:') and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert not wav.any() and not mel.any() and not picks.any()          # a refused call wrote nothing
    assert call()[0] == 0
    # the Python layer: no utterance long enough; a crop the featuriser cannot pad
    with pytest.raises(ValueError, match='none of the 2 utterances has 5000 samples'):
        train.DeviceDataset([np.zeros(1200, np.float32), np.zeros(4999, np.float32)], 5000)
    with pytest.raises(ValueError, match='need more than 1024'):
        train.DeviceDataset([np.zeros(1200, np.float32)], 1000).batch(0, 1)


def test_from_tfrecord(tmp_path):
    import torch
    from nsynth_wavenet_amd import train
    from nsynth_wavenet_amd.auxilaries import reader
    path = str(tmp_path / 'p.tfrecord')
    pool = _pool(1200)
    reader.write_tfrecord(path, [('u{}'.format(i), a) for i, a in enumerate(pool)])
    ds = train.DeviceDataset.from_tfrecord(path, 1200, seed=SEED)
    out, want = ds.batch(11, 3, mel_rand=True), _batch(1200, 3)
    for key in ('wav', 'mel', 'mel_rand', 'picks'):
        assert torch.equal(out[key], want[key]), key
