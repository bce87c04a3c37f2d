"""Drop-in for the reference's build_dataset.py: a directory of .wav files -> the TFRecord the training CLIs read.

    python build_dataset.py --wave_dir WAVS --save_path train.tfrecord [--sample_rate 16000 --min_len 16000 --num_workers 10]

One tf.train.Example per file, in sorted file order: 'audio_id' (the file name without its extension), 'audio' (float32
samples in [-1, 1], zero-padded at the end to --min_len) and 'length' (the length before padding), written by
nsynth_wavenet_amd/auxilaries/reader.py.  16-bit, 32-bit and float PCM files are read with scipy.io.wavfile where it is
installed, 16-bit files with the standard `wave` module otherwise; the first channel of a multi-channel file is taken.
NOT done: resampling (the reference resamples through librosa.load).  A file whose rate is not --sample_rate is refused by
name: resample it first.
"""
import argparse
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from nsynth_wavenet_amd.auxilaries import reader


def read_wav(path):
    """(float32 samples in [-1, 1], sample rate)"""
    try:
        from scipy.io import wavfile
    except ImportError:
        wavfile = None
    if wavfile is not None:
        sr, data = wavfile.read(path)
        if data.ndim > 1:
            data = data[:, 0]
        if data.dtype.kind == 'i':
            data = data.astype(np.float32) / float(2 ** (8 * data.dtype.itemsize - 1))
        elif data.dtype.kind == 'u':                                # 8-bit PCM is unsigned
            data = (data.astype(np.float32) - 128.0) / 128.0
        return data.astype(np.float32), int(sr)
    import wave
    with wave.open(path, 'rb') as f:
        if f.getsampwidth() != 2:
            raise ValueError('{}: {}-byte samples; without scipy only 16-bit PCM is read'.format(path, f.getsampwidth()))
        sr, ch = f.getframerate(), f.getnchannels()
        data = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2').reshape(-1, ch)[:, 0]
    return (data.astype(np.float32) / 32768.0), int(sr)


def pad_wave(waveform, min_len):
    """zeros appended up to min_len samples; a longer signal is returned as it is"""
    short = int(min_len) - waveform.shape[0]
    return np.concatenate([waveform, np.zeros(short, waveform.dtype)]) if short > 0 else waveform


def make_example(path, sr, min_len):
    """(audio_id, padded samples, length before padding)"""
    waveform, rate = read_wav(path)
    if rate != sr:
        raise ValueError('{}: sample rate {} is not --sample_rate {} (resampling is not done here: resample the file '
                         'first)'.format(path, rate, sr))
    return os.path.splitext(os.path.basename(path))[0], pad_wave(waveform, min_len), waveform.shape[0]


def build_dataset(wave_dir, save_path, sr=16000, min_len=16000, num_workers=10):
    wave_files = sorted(glob.glob(os.path.join(wave_dir, '*.wav')))
    if not wave_files:
        raise ValueError('no .wav file in {}'.format(wave_dir))
    with ThreadPoolExecutor(max_workers=max(1, int(num_workers))) as ex:
        items = list(ex.map(lambda p: make_example(p, sr, min_len), wave_files))
    reader.write_tfrecord(save_path, items)
    hours = sum(n for _, _, n in items) / float(sr) / 3600.0
    padded = sum(1 for _, a, n in items if a.shape[0] != n)
    print('{}: {} utterances, {:.5f} hours of audio, {} padded to {} samples'.format(save_path, len(items), hours, padded, min_len))
    return len(items)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--wave_dir', required=True, help='directory of the .wav files')
    parser.add_argument('--save_path', required=True, help='TFRecord file to write')
    parser.add_argument('--sample_rate', default=16000, type=int, help='the rate every file must have (Hz)')
    parser.add_argument('--min_len', default=16000, type=int, help='shorter files are zero-padded to this many samples')
    parser.add_argument('--num_workers', default=10, type=int, help='threads that read the files')
    args = parser.parse_args()
    build_dataset(args.wave_dir, args.save_path, args.sample_rate, args.min_len, args.num_workers)
