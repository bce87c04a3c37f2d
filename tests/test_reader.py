"""Host tests of the training set's TFRecord reader / writer (nsynth_wavenet_amd/auxilaries/reader.py), of build_dataset.py
and of the numpy twin of the device-side batch picks (train.batch_picks)."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from nsynth_wavenet_amd import tf_bundle, train
from nsynth_wavenet_amd.auxilaries import reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One record assembled by hand: the Example of audio_id 'a1', audio [0.5, -1.0], length 2 -- with the features in another
# order than the writer's and the int64 NOT packed, which a parser of the format has to accept too.
HAND = bytes.fromhex(
    '3d 00 00 00 00 00 00 00'                      # uint64 length = 61
    '60 49 f1 ec'                                  # masked crc32c of those eight bytes
    '0a 3b'                                        # Example.features (field 1), 59 bytes
    '0a 12 0a 08 61 75 64 69 6f 5f 69 64'          #   map entry, 18 bytes: key (1) = "audio_id"
    '12 06 0a 04 0a 02 61 31'                      #     value (2): Feature.bytes_list (1) { value (1) = "a1" }
    '0a 0e 0a 06 6c 65 6e 67 74 68'                #   map entry, 14 bytes: key = "length"
    '12 04 1a 02 08 02'                            #     Feature.int64_list (3) { value (1) = varint 2 }
    '0a 15 0a 05 61 75 64 69 6f'                   #   map entry, 21 bytes: key = "audio"
    '12 0c 0a 0a 0a 08 00 00 00 3f 00 00 80 bf'    #     Feature.bytes_list { value = float32 0.5, -1.0 little endian }
    '26 06 1f 36')                                 # masked crc32c of the 61 payload bytes


def _utterances():
    rs = np.random.RandomState(4)
    return [('utt_{}'.format(i), rs.uniform(-1, 1, n).astype(np.float32), m) for i, (n, m) in enumerate([(5, 5), (1200, 700), (333, 333)])]


def test_crc32c_check_value():
    """the CRC the hand-assembled record rests on: CRC-32C of '123456789' is 0xE3069283 (RFC 3720 B.4)"""
    assert tf_bundle.crc32c(b'123456789') == 0xE3069283


def test_round_trip(tmp_path):
    path = str(tmp_path / 'a.tfrecord')
    items = _utterances()
    assert reader.write_tfrecord(path, items) == 3
    got = list(reader.read_tfrecord(path))
    assert len(got) == 3
    for (aid, audio, length), (gid, gaudio, glength) in zip(items, got):
        assert gid == aid.encode() and glength == length
        assert gaudio.dtype == np.float32 and np.array_equal(gaudio.view(np.int32), audio.view(np.int32))


def test_hand_assembled_record(tmp_path):
    path = str(tmp_path / 'hand.tfrecord')
    with open(path, 'wb') as f:
        f.write(HAND + HAND)
    got = list(reader.read_tfrecord(path))
    assert len(got) == 2
    for aid, audio, length in got:
        assert aid == b'a1' and length == 2
        assert audio.dtype == np.float32 and audio.tolist() == [0.5, -1.0]
    # and the writer's own bytes parse to the same values (it packs the int64 and sorts the keys)
    assert reader.decode_example(reader.encode_example('a1', [0.5, -1.0], 2))[0] == b'a1'


@pytest.mark.parametrize('where', ['data', 'length', 'data_crc'])
def test_flipped_byte_raises(tmp_path, where):
    path = str(tmp_path / 'bad.tfrecord')
    raw = bytearray(HAND)
    raw[{'data': 40, 'length': 1, 'data_crc': len(raw) - 1}[where]] ^= 0x10
    with open(path, 'wb') as f:
        f.write(bytes(raw))
    with pytest.raises(ValueError, match='checksum mismatch'):
        list(reader.read_tfrecord(path))


@pytest.mark.parametrize('keep', [5, 12, 40, len(HAND) - 1, len(HAND) + 3])
def test_truncated_file_raises(tmp_path, keep):
    path = str(tmp_path / 'cut.tfrecord')
    with open(path, 'wb') as f:
        f.write((HAND + HAND)[:keep])
    with pytest.raises(ValueError, match='truncated'):
        list(reader.read_tfrecord(path))


def test_missing_feature_is_named():
    with pytest.raises(ValueError, match='audio_id'):
        reader.decode_example(bytes.fromhex('0a 10 0a 0e 0a 06 6c 65 6e 67 74 68 12 04 1a 02 08 02'))


def _write_wav(path, samples, rate):
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.asarray(samples, '<i2').tobytes())


def test_build_dataset(tmp_path):
    """16-bit wavs -> float32 / 32768, zero-padded to --min_len, 'length' the length before padding, sorted file order; a file
    of another rate is refused by name"""
    wavs = tmp_path / 'wavs'
    wavs.mkdir()
    rs = np.random.RandomState(1)
    a, b = rs.randint(-32768, 32768, 300), rs.randint(-32768, 32768, 90)
    _write_wav(str(wavs / 'b_long.wav'), a, 16000)
    _write_wav(str(wavs / 'a_short.wav'), b, 16000)
    out = str(tmp_path / 'train.tfrecord')
    cmd = [sys.executable, os.path.join(ROOT, 'build_dataset.py'), '--wave_dir', str(wavs), '--save_path', out, '--min_len', '128']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = list(reader.read_tfrecord(out))
    assert [g[0] for g in got] == [b'a_short', b'b_long'] and [g[2] for g in got] == [90, 300]
    assert got[0][1].shape == (128,) and np.array_equal(got[0][1][:90], b.astype(np.float32) / 32768) and not got[0][1][90:].any()
    assert np.array_equal(got[1][1], a.astype(np.float32) / 32768)
    _write_wav(str(wavs / 'c_8k.wav'), b, 8000)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and 'c_8k.wav' in r.stderr and 'sample rate 8000' in r.stderr


# ---- batch_picks ----
LENGTHS, L = [500, 1600, 1201, 1200, 4000], 1200


@pytest.fixture(scope='module')
def picks():
    """4096 steps x B = 8 under seed 0: [4096, 8, 2]"""
    return np.stack([train.batch_picks(0, k, 8, LENGTHS, L) for k in range(4096)])


def test_picks_stay_inside(picks):
    u, start = picks[..., 0].ravel(), picks[..., 1].ravel()
    assert picks.dtype == np.int64
    assert not (u == 0).any() and set(u.tolist()) == {1, 2, 3, 4}
    assert (start[u == 3] == 0).all()
    assert (start >= 0).all() and (start <= np.asarray(LENGTHS)[u] - L).all()
    assert set(start[u == 2].tolist()) == {0, 1}
    assert start[u == 4].max() > 2700 and start[u == 4].min() < 100


def test_picks_are_uniform(picks):
    """Fixed seed, deterministic: each of the 4 eligible utterances' share of the 32 768 picks, and each of 8 equal bins of
    utterance 4's 2801 starts, within 5 standard deviations of the binomial under the uniform law."""
    u, start = picks[..., 0].ravel(), picks[..., 1].ravel()
    n = u.size
    for i in (1, 2, 3, 4):
        z = ((u == i).sum() - n / 4.0) / np.sqrt(n * 0.25 * 0.75)
        print('utterance {}: {:+.2f} sd'.format(i, z))
        assert abs(z) <= 5
    s4 = start[u == 4]
    edges = np.linspace(0, 2801, 9)
    for k in range(8):
        lo, hi = int(np.ceil(edges[k])), int(np.ceil(edges[k + 1]))          # bin k holds the starts lo .. hi - 1
        p = (hi - lo) / 2801.0
        z = (((s4 >= lo) & (s4 < hi)).sum() - s4.size * p) / np.sqrt(s4.size * p * (1 - p))
        print('start bin {}: {:+.2f} sd'.format(k, z))
        assert abs(z) <= 5


def test_picks_depend_on_stream_step_seed_not_on_B():
    base = train.batch_picks(3, 17, 8, LENGTHS, L)
    assert not np.array_equal(base, train.batch_picks(3, 17, 8, LENGTHS, L, stream=1))
    assert not np.array_equal(base, train.batch_picks(3, 18, 8, LENGTHS, L))
    assert not np.array_equal(base, train.batch_picks(4, 17, 8, LENGTHS, L))
    assert not np.array_equal(base, train.batch_picks(3 + 2 ** 32, 17, 8, LENGTHS, L))        # the key's high word
    assert not np.array_equal(base, train.batch_picks(3, 17 + 2 ** 32, 8, LENGTHS, L))        # the counter's second word
    assert np.array_equal(base, train.batch_picks(3, 17, 8, LENGTHS, L))
    assert np.array_equal(train.batch_picks(3, 17, 29, LENGTHS, L)[:8], base)
    with pytest.raises(ValueError, match='no utterance'):
        train.batch_picks(0, 0, 2, [10, 20], 100)
