"""TFRecord reader / writer for the training set, without TensorFlow.

The reference's build_dataset.py writes one tf.train.Example per utterance into a TFRecord file and
auxilaries/reader.py:39-42 parses it with FEATURES = {'audio_id': string, 'audio': string (raw little-endian float32
samples), 'length': int64 (the length before padding)}.  This module restates both formats:

  record   uint64 length | uint32 masked crc32c(length bytes) | data | uint32 masked crc32c(data), little endian, the
           CRC and its mask being tf_bundle.crc32c / tf_bundle.mask_crc;
  payload  Example { features (1): Features { feature (1): map entry { key (1): string, value (2): Feature {
           bytes_list (1): BytesList { value (1) } | int64_list (3): Int64List { value (1), packed or not } } } } }.

Validated only against itself (writer <-> reader round trip) and a hand-assembled record spelled out in
tests/test_reader.py: no TensorFlow-written file is available offline.  The device-resident dataset built from such a
file is train.DeviceDataset.
"""
import struct

import numpy as np

from ..tf_bundle import _get_varint, _parse_proto, _put_varint, _signed64, crc32c, mask_crc

FEATURES = ('audio_id', 'audio', 'length')


def _ld(field, payload):
    """length-delimited field"""
    return _put_varint(field << 3 | 2) + _put_varint(len(payload)) + payload


def encode_example(audio_id, audio, length):
    """The serialized tf.train.Example of one utterance (keys in sorted order, as protobuf serialises a map
    deterministically)."""
    if isinstance(audio_id, str):
        audio_id = audio_id.encode('utf-8')
    raw = np.ascontiguousarray(np.asarray(audio, np.float32)).astype('<f4').tobytes()
    feats = {b'audio': _ld(1, _ld(1, raw)),                                          # Feature.bytes_list
             b'audio_id': _ld(1, _ld(1, bytes(audio_id))),
             b'length': _ld(3, _ld(1, _put_varint(int(length))))}                    # Feature.int64_list, packed
    entries = b''.join(_ld(1, _ld(1, k) + _ld(2, feats[k])) for k in sorted(feats))
    return _ld(1, entries)


def _first(fields, number, what):
    for f, wt, v in fields:
        if f == number:
            return wt, v
    raise ValueError('TFRecord example: no {}'.format(what))


def decode_example(buf):
    """serialized Example -> (audio_id bytes, float32 array, length)"""
    wt, features = _first(_parse_proto(buf), 1, 'features')
    got = {}
    for f, wt, entry in _parse_proto(features):
        if f != 1 or wt != 2:
            continue
        kv = _parse_proto(entry)
        key = _first(kv, 1, 'feature key')[1]
        got[key.decode('utf-8', 'replace')] = _parse_proto(_first(kv, 2, 'feature value')[1])
    missing = [k for k in FEATURES if k not in got]
    if missing:
        raise ValueError('TFRecord example lacks the feature(s) {} (has {})'.format(missing, sorted(got)))

    def bytes_value(name):
        wt, lst = _first(got[name], 1, "a bytes_list in '{}'".format(name))
        return _first(_parse_proto(lst), 1, "a value in '{}'".format(name))[1]

    wt, lst = _first(got['length'], 3, "an int64_list in 'length'")
    wt, v = _first(_parse_proto(lst), 1, "a value in 'length'")
    length = _signed64(_get_varint(v, 0)[0] if wt == 2 else v)       # packed (proto3 writers) or one varint per value
    raw = bytes_value('audio')
    if len(raw) % 4:
        raise ValueError("TFRecord example: 'audio' holds {} bytes, not a whole number of float32 samples".format(len(raw)))
    return bytes_value('audio_id'), np.frombuffer(raw, dtype='<f4').astype(np.float32), int(length)


def read_records(path):
    """Yield the payload of every record of a TFRecord file; ValueError on a CRC mismatch or a truncated file."""
    with open(path, 'rb') as f:
        n = 0
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise ValueError('{}: truncated in the header of record {}'.format(path, n))
            length, crc = struct.unpack('<QI', head)
            if mask_crc(crc32c(head[:8])) != crc:
                raise ValueError('{}: length checksum mismatch in record {}'.format(path, n))
            body = f.read(length + 4)
            if len(body) < length + 4:
                raise ValueError('{}: truncated in record {} ({} of {} bytes)'.format(path, n, len(body), length + 4))
            if mask_crc(crc32c(body[:length])) != struct.unpack('<I', body[length:])[0]:
                raise ValueError('{}: data checksum mismatch in record {}'.format(path, n))
            yield body[:length]
            n += 1


def read_tfrecord(path):
    """Yield (audio_id bytes, float32 samples, length before padding) for every utterance of the file."""
    for payload in read_records(path):
        yield decode_example(payload)


def write_tfrecord(path, items):
    """items: (audio_id, samples, length) or (audio_id, samples) -> the file read_tfrecord reads.  Returns the count."""
    n = 0
    with open(path, 'wb') as f:
        for item in items:
            audio_id, audio = item[0], np.asarray(item[1], np.float32)
            payload = encode_example(audio_id, audio, item[2] if len(item) > 2 else audio.shape[0])
            head = struct.pack('<Q', len(payload))
            f.write(head + struct.pack('<I', mask_crc(crc32c(head))) + payload + struct.pack('<I', mask_crc(crc32c(payload))))
            n += 1
    return n
