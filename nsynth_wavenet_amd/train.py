"""Training on the device.  The teacher: train_wavenet.py's AdamOptimizer(lr, epsilon=1e-8), its optional
clip_by_global_norm and its ExponentialMovingAverage(0.9999, num_updates=global_step) on top of
Wavenet.loss_and_weight_grads, with the updated weights re-packed into the SAME handle by Engine.teacher_set_weights.  No
weight and no gradient crosses to the host during a step.

    teacher = Wavenet(hparams).load_weights(w)
    trainer = TeacherTrainer(teacher, w, lr={0: 2e-4, 90000: 6e-5})
    for batch in batches:                       # {'wav': [B,T], 'mel': [B,F,80]}
        out = trainer.step(batch)               # {'loss', 'log_probs', 'grad_norm'}: device tensors
    np.savez('eval.npz', **trainer.weights(ema=True))

The student: train_parallel_wavenet.py's loop -- the same optimiser and shadow over the variables of the flows
and of the deconv stacks the student owns -- on top of ParallelWavenet.loss_and_weight_grads and Engine.iaf_set_weights.

    student = ParallelWavenet(hparams, teacher=teacher).load_weights(w)
    trainer = StudentTrainer(student, w, lr={0: 2e-4, 90000: 6e-5})
    for batch in batches:                       # {'wav': [B,T'], 'mel': [B,F,80]} (+ 'mel_rand')
        out = trainer.step(batch)               # calculate_loss's entries and 'grad_norm': device tensors

The batches: DeviceDataset keeps the training set on the device and cuts the batch of step k from it in one
launch, a pure function of (seed, k); trainer.save(logdir) / trainer.restore(logdir) write and read a TF V2 checkpoint with
the optimiser state, so that a restored trainer continues with the bits of the uninterrupted run.

    ds = DeviceDataset.from_tfrecord(train_path, hparams.wave_length, seed=0)
    while trainer.global_step < num_iters:
        out = trainer.step(ds.batch(trainer.global_step, batch_size))
    trainer.save(logdir)

train_wavenet.py / train_parallel_wavenet.py (train_cli.py) are this loop behind the reference's command lines.

Shards: trainer.step(batch, micro_batch=m) runs the step in B / m shards and averages their gradients in a
fixed order (Engine.grad_combine); a trainer built with data_parallel=True under torch.distributed spreads the shards over
the ranks.  The result depends on (B, m) alone, so a run on N GPUs has the bits of the run on one.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from . import weights as wts
from .engine import NotConverged, adam_ema_step, grad_sumsq


def scheduled_lr(lr, global_step):
    """The learning rate train_wavenet.py:141-144 builds from a {step: lr} dict (wavenet.py:100): schedule[0], replaced in
    the dict's own order by every entry whose key is <= global_step.  A float is a constant rate."""
    if not isinstance(lr, dict):
        return float(lr)
    if 0 not in lr:
        raise ValueError('an lr schedule needs an entry for step 0 (train_wavenet.py:141)')
    cur = lr[0]
    for key, value in lr.items():
        if not global_step < key:
            cur = value
    return float(cur)


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words (broadcast against each other) -> the four output words"""
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)]
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2                   # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def dropout_threshold(rate):
    """min(2^32 - 1, floor(rate 2^32 + 0.5)): an element is kept where its 32-bit hash word is >= this"""
    if not 0.0 <= rate < 1.0:
        raise ValueError('dropout rate {} is outside [0, 1)'.format(rate))
    return min(2 ** 32 - 1, int(math.floor(float(rate) * 2.0 ** 32 + 0.5)))


def dropout_keep(seed, site, B, C, T, rate):
    """The dropout mask of the device-side training step, on the host: bool [B, T, C], True = kept.
    Element (b, c, t) of site `site` is kept where word t % 4 of Philox4x32-10(key = the 64-bit seed, counter =
    (t // 4, c, site, b)) is >= dropout_threshold(rate).  The bit depends on (seed, site, b, c, t) and the rate alone, so a
    larger B, C or T extends the mask without changing it.  Sites: dropout_inputs 0 = conv_dropout (l, C = width),
    1 = skip_dropout (s, C = skip_width); dropout_all 0 = conv_dropout, i = res_dropout_i.  Engine.teacher_dropout_keep
    returns the same bits from the device function the kernels call."""
    seed = int(seed) & (2 ** 64 - 1)
    thr = dropout_threshold(rate)
    T4 = (int(T) + 3) // 4
    b = np.arange(int(B), dtype=np.uint64)[:, None, None]
    t4 = np.arange(T4, dtype=np.uint64)[None, :, None]
    c = np.arange(int(C), dtype=np.uint64)[None, None, :]
    words = _philox4x32_10(t4, c, np.uint64(int(site)), b, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(np.broadcast_arrays(*words), axis=2)           # [B, T4, 4, C]
    return (words >= np.uint64(thr)).reshape(int(B), 4 * T4, int(C))[:, :int(T)]


def dropout_step_seed(base, step):
    """The mask seed of training step `step` (0 = the first) under the trainer's dropout_seed `base`: the 64-bit value
    (base + step * 0x9E3779B97F4A7C15) mod 2^64.  The multiplier is odd, so for one base the seeds of 2^64 consecutive steps
    are distinct, and a trainer resumed at step n continues the sequence it would have run."""
    return (int(base) + int(step) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)


_M64 = 2 ** 64 - 1
MAX_SHARDS = 64                     # wn_grad_combine's bound on the rows of one call
SCALAR_KEYS = ('loss', 'kl_loss', 'H_Ps', 'H_Ps_Pt', 'power_loss', 'contrastive_loss')
ROW_SCALARS = 8                     # scalar slots behind the gradients of a row: SCALAR_KEYS in order, then zero padding
ROW_INPUTS = ('wav', 'mel', 'mel_rand')


def _mix64(x):
    """the finaliser of SplitMix64: a bijection of the 64-bit words"""
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def shard_seed(seed, j):
    """The seed of shard j of a step whose seed is `seed`, a pure function of the two: `seed` itself for
    j = 0, so that a step of one shard draws what the unsharded step draws, and for j > 0 the 64-bit value
    mix(mix(seed mod 2^64) + j mod 2^64) with mix the finaliser of SplitMix64.  No plain seed + j: the seeds of consecutive
    steps are seed + k (the student) or base + k * odd (dropout_step_seed), and an additive shard seed would hand a shard
    of one step the draws of a neighbouring step's.  mix is a bijection, so for one j distinct seeds stay distinct."""
    seed, j = int(seed), int(j)
    if j < 0:
        raise ValueError('shard_seed: shard index {} is negative'.format(j))
    if j == 0:
        return seed
    return _mix64((_mix64(seed & _M64) + j) & _M64)


def combine_np(rows):
    """wn_grad_combine on the host: (((rows[0] + rows[1]) + rows[2]) + ...) * (float32(1) / float32(S)) in float32, one
    rounding per operation, over the S = len(rows) arrays of equal shape.  The bits of Engine.grad_combine."""
    rows = [np.asarray(r, np.float32) for r in rows]
    if not 1 <= len(rows) <= MAX_SHARDS:
        raise ValueError('combine_np: {} rows; the combine takes 1 to {}'.format(len(rows), MAX_SHARDS))
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = (acc + r).astype(np.float32)
    return (acc * (np.float32(1) / np.float32(len(rows)))).astype(np.float32)


def shard_plan(B, m, world=1, rank=0):
    """How a step on B rows is cut: micro-batches of m rows give S = B / m shards, shard j being rows
    [j m, (j + 1) m), and rank `rank` of `world` computes the contiguous shards dist.shard_range(S, rank, world).
    Returns (S, (first shard, one past the last), (first row, one past the last)) of that rank.  ValueError for B % m != 0,
    for more than MAX_SHARDS shards and for S % world != 0."""
    from .dist import shard_range
    B, m, world, rank = int(B), int(m), int(world), int(rank)
    if B < 1 or m < 1 or B % m != 0:
        raise ValueError('a batch of B = {} rows does not split into micro-batches of m = {}: B % m must be 0'.format(B, m))
    S = B // m
    if S > MAX_SHARDS:
        raise ValueError('B = {} rows in micro-batches of m = {} are S = {} shards; a step takes at most {}'.format(B, m, S, MAX_SHARDS))
    if world < 1 or not 0 <= rank < world:
        raise ValueError('rank {} is outside a world of {}'.format(rank, world))
    if S % world != 0:
        raise ValueError('B = {} rows in micro-batches of m = {} are S = {} shards, which W = {} ranks do not share evenly: '
                         'S % W must be 0'.format(B, m, S, world))
    lo, hi = shard_range(S, rank, world)
    return S, (lo, hi), (lo * m, hi * m)


def batch_picks(seed, step, B, lengths, L, stream=0):
    """The picks of the device-side batch (wn_train_batch), on the host: int64 [B, 2] = (utterance index,
    start) of every row.  Row b of stream `stream` takes the words r of Philox4x32-10(key = the 64-bit seed, counter =
    (step lo, step hi, b, stream)); with `eligible` the indices of the utterances of at least L samples, in order,
    u = eligible[(r0 * len(eligible)) >> 32] and start = (r1 * (lengths[u] - L + 1)) >> 32.  A function of (seed, step, b,
    stream) and the lengths alone: a larger B extends the picks without changing them."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    L = int(L)
    eligible = np.nonzero(lengths >= L)[0]
    if eligible.size < 1:
        raise ValueError('batch_picks: no utterance has {} samples (the longest has {})'.format(L, int(lengths.max()) if lengths.size else 0))
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    b = np.arange(int(B), dtype=np.uint64)
    r = _philox4x32_10(np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32), b, np.uint64(int(stream)), seed & 0xFFFFFFFF, seed >> 32)
    r0, r1 = (np.broadcast_to(w, b.shape).astype(np.uint64) for w in r[:2])
    u = eligible[((r0 * np.uint64(eligible.size)) >> np.uint64(32)).astype(np.int64)]
    span = (lengths[u] - L + 1).astype(np.uint64)
    start = ((r1 * span) >> np.uint64(32)).astype(np.int64)
    return np.stack([u.astype(np.int64), start], axis=1)


class DeviceDataset(object):
    """The training set on the device: every utterance back to back in one float32 pool, and the batch of a step cut from
    it and featurised by one launch of wn_train_batch (csrc/wn_batch.hip).  Replaces the reference's TFRecord queue, random
    crop and shuffle_batch (auxilaries/reader.py:61-108): the same marginal distribution -- an utterance uniformly among
    those of at least `length` samples, a start uniformly among those tf.random_crop can return -- as a function of
    (seed, step), so a resumed run sees the batches of the uninterrupted one.

    utterances: a list of 1-d float arrays.  length: the crop, hparams.wave_length (more than 1024 samples)."""

    def __init__(self, utterances, length, seed=0, device=None):
        self.length, self.seed = int(length), int(seed) & (2 ** 64 - 1)
        self.utterances = [np.ascontiguousarray(np.asarray(u, np.float32).reshape(-1)) for u in utterances]
        self.lengths = np.array([u.shape[0] for u in self.utterances], np.int64)
        eligible = np.nonzero(self.lengths >= self.length)[0].astype(np.int32)
        if eligible.size < 1:
            raise ValueError('DeviceDataset: none of the {} utterances has {} samples (the longest has {})'.format(
                len(self.utterances), self.length, int(self.lengths.max()) if self.lengths.size else 0))
        self.lib = _lib.load()
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.pool = torch.from_numpy(np.concatenate(self.utterances)).to(self.device)
        self.utt_off = torch.from_numpy(offsets).to(self.device)
        self.utt_len = torch.from_numpy(self.lengths.copy()).to(self.device)
        self.eligible = torch.from_numpy(eligible).to(self.device)
        self.frames = int(self.lib.wn_mel_frames(self.length))

    @classmethod
    def from_tfrecord(cls, path, length, seed=0, device=None):
        """Every utterance of a TFRecord written by build_dataset.py (auxilaries/reader.py), padded as stored."""
        from .auxilaries import reader
        return cls([audio for _, audio, _ in reader.read_tfrecord(path)], length, seed=seed, device=device)

    def batch(self, step, batch_size, mel_rand=False):
        """{'wav': [B, length], 'mel': [B, frames, 80], 'picks': int64 [n_streams, B, 2]} of step `step`, with mel_rand=True
        also 'mel_rand' [B, frames, 80] (the mel of a second, unrelated draw): device tensors, enqueued on the current
        stream without a host synchronisation."""
        B, ns = int(batch_size), 2 if mel_rand else 1
        with torch.cuda.device(self.device):
            wav = torch.empty(B, self.length, dtype=torch.float32, device=self.device)
            mel = torch.empty(ns, B, self.frames, 80, dtype=torch.float32, device=self.device)
            picks = torch.empty(ns, B, 2, dtype=torch.int64, device=self.device)
            _lib.check(self.lib.wn_train_batch(self.pool.data_ptr(), self.utt_off.data_ptr(), self.utt_len.data_ptr(),
                                               self.eligible.data_ptr(), int(self.eligible.numel()), B, self.length, self.seed,
                                               int(step) & (2 ** 64 - 1), ns, wav.data_ptr(), mel.data_ptr(), picks.data_ptr(),
                                               torch.cuda.current_stream(self.device).cuda_stream))
        out = {'wav': wav, 'mel': mel[0], 'picks': picks}
        if mel_rand:
            out['mel_rand'] = mel[1]
        return out

    def host_batch(self, step, batch_size, mel_rand=False):
        """The same batch by the host route, as numpy arrays: batch_picks, slices of the utterances and
        auxilaries.mel_extractor.batch_melspectrogram (float64 FFT) -- what the tests and the benchmark compare with."""
        from .auxilaries import mel_extractor
        picks = [batch_picks(self.seed, step, batch_size, self.lengths, self.length, stream=s) for s in range(2 if mel_rand else 1)]
        crops = [np.stack([self.utterances[u][t:t + self.length] for u, t in p]) for p in picks]
        out = {'wav': crops[0], 'mel': mel_extractor.batch_melspectrogram(crops[0]), 'picks': np.stack(picks)}
        if mel_rand:
            out['mel_rand'] = mel_extractor.batch_melspectrogram(crops[1])
        return out


# ---- checkpoints: the keys tf.train.Saver writes for the reference's training graph ----
ADAM_M, ADAM_V = '/Adam', '/Adam_1'


def checkpoint_tensors(trained, frozen, global_step, beta1=0.9, beta2=0.999):
    """{checkpoint key: array} of one training state.  trained: {variable: (value, m, v, shadow)} -> '<var>', '<var>/Adam',
    '<var>/Adam_1', '<var>/ExponentialMovingAverage'; frozen: {variable: value} under the plain name only; 'global_step'
    (int32) and the informational 'beta1_power' / 'beta2_power' (float32, beta^global_step)."""
    out = {}
    for name, (p, m, v, e) in trained.items():
        out[name], out[name + ADAM_M], out[name + ADAM_V], out[name + wts.EMA] = (np.asarray(a, np.float32) for a in (p, m, v, e))
    for name, a in frozen.items():
        out[name] = np.asarray(a, np.float32)
    out['global_step'] = np.array(int(global_step), np.int32)
    out['beta1_power'] = np.array(float(beta1) ** int(global_step), np.float32)
    out['beta2_power'] = np.array(float(beta2) ** int(global_step), np.float32)
    return out


def write_checkpoint(logdir, tensors):
    """model.ckpt-<global_step> (a TF V2 bundle) in logdir and the `checkpoint` state file naming it; returns the prefix"""
    from . import tf_bundle
    os.makedirs(logdir, exist_ok=True)
    name = 'model.ckpt-{:d}'.format(int(tensors['global_step']))
    prefix = tf_bundle.write_bundle(os.path.join(logdir, name), tensors)
    with open(os.path.join(logdir, 'checkpoint'), 'wt') as f:
        f.write('model_checkpoint_path: "{0}"\nall_model_checkpoint_paths: "{0}"\n'.format(name))
    return prefix


def resolve_checkpoint(prefix_or_logdir):
    """a checkpoint prefix as it is, a directory -> its latest checkpoint (weights.latest_checkpoint)"""
    if os.path.isdir(prefix_or_logdir):
        prefix = wts.latest_checkpoint(prefix_or_logdir)
        if prefix is None:
            raise ValueError('no checkpoint found in {}'.format(prefix_or_logdir))
        return prefix
    return prefix_or_logdir


def checkpoint_weights(prefix_or_logdir, hp, kind=None):
    """{variable: value} of a training checkpoint under the PLAIN names -- the weights a run continues from, where
    weights.load_checkpoint prefers the shadows (what generation wants)."""
    from . import tf_bundle
    prefix = resolve_checkpoint(prefix_or_logdir)
    r = tf_bundle.BundleReader(prefix)
    out = {}
    for name, shape in wts.expected_variables(hp, kind):
        if not r.has_tensor(name):
            raise KeyError('checkpoint {} lacks {}'.format(prefix, name))
        a = r.get_tensor(name)
        if a.size != int(np.prod(shape)):
            raise ValueError('checkpoint {}: {} has shape {}, the model expects {}'.format(prefix, name, list(a.shape), list(shape)))
        out[name] = np.asarray(a, np.float32).reshape(shape)
    return out


class _TrainerType(type):
    """Takes the construction keyword every trainer shares, data_parallel=, before __init__ runs, so that the __init__
    signatures of the three trainers stay what their callers know.  data_parallel=True needs an initialised
    torch.distributed process group: the trainer then computes its rank's shards of every step."""

    def __call__(cls, *args, data_parallel=False, **kw):
        world, rank = 1, 0
        if data_parallel:
            import torch.distributed as td
            if cls.DATA_PARALLEL_REFUSAL:
                raise ValueError('{}: data_parallel=True is not supported: {}'.format(cls.__name__, cls.DATA_PARALLEL_REFUSAL))
            if not (td.is_available() and td.is_initialized()):
                raise ValueError('{}: data_parallel=True needs an initialised torch.distributed process group '
                                 '(dist.init_process_group)'.format(cls.__name__))
            world, rank = td.get_world_size(), td.get_rank()
        self = cls.__new__(cls)
        self.data_parallel, self.world, self.rank = bool(data_parallel), world, rank
        self.__init__(*args, **kw)
        return self


class _DeviceTrainer(object, metaclass=_TrainerType):
    """What the trainers share: the flat (p, m, v, ema) buffers of one or more gradient tables scattered from a weights
    dict, the Adam / EMA update with its learning-rate bookkeeping, the sharded step, and weights() /
    use_ema() / use_weights().  A subclass sets self.eng and implements _repack(bufs) and _shard(rows, j, extra).

    Shards: step(inputs, micro_batch=m) cuts the B rows of every per-row input ('wav', 'mel', 'mel_rand', a `noise`) into
    S = B / m shards (at most 64), evaluates each by the model's own public call under train.shard_seed(step seed, j), and
    writes its flat gradients and scalars into row j of one [S, row_floats] buffer: gradient buffer i at row_offsets[i] (the
    table's order, each start rounded up to 4 floats), then ROW_SCALARS slots for SCALAR_KEYS.  Engine.grad_combine reduces
    the rows in shard order into row 0, which feeds the update.  The result depends on (B, m) alone.

    data_parallel=True (construction keyword, with torch.distributed initialised, world size W): every rank is handed the
    full batch, computes the shards dist.shard_range(S, rank, W) (S % W == 0) and the ranks exchange rows by one all-gather;
    the combine, Adam and the re-pack then run on every rank on identical bits, so a run on W ranks has the bits of the
    run on one with the same (B, m).  save() writes on rank 0 only; restore() is every rank's."""
    DATA_PARALLEL_REFUSAL = None
    data_parallel, world, rank = False, 1, 0
    record_events = False             # True: step keeps (start, exchanged, combined) device events in last_events
    last_events = None

    def _init_optimiser(self, lr, beta1, beta2, eps, ema_decay, clip_norm):
        self.lr, self.beta1, self.beta2, self.eps = lr, float(beta1), float(beta2), float(eps)
        self.ema_decay = float(ema_decay)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        scheduled_lr(lr, 0)

    def _init_buffers(self, weights, tables, sizes):
        """tables: [[(tf name, float offset, TF shape)]], sizes: the library's float count of each"""
        who = type(self).__name__
        dev = self.eng.device
        self.tables = tables
        self.p, self.m, self.v, self.ema = [], [], [], []
        for tab, size in zip(tables, sizes):
            flat = np.zeros(size, np.float32)        # the library's own count; anything a table does not cover stays zero
            for name, off, shape in tab:
                a = np.asarray(weights[name], np.float32)
                if a.size != int(np.prod(shape)):
                    raise ValueError('{}: {} has {} values, the model expects shape {}'.format(who, name, a.size, shape))
                flat[off:off + a.size] = a.reshape(-1)          # Saver(reshape=True): same element count
            p = torch.from_numpy(flat).to(dev)
            self.p.append(p)
            self.m.append(torch.zeros_like(p))
            self.v.append(torch.zeros_like(p))
            self.ema.append(p.clone())
        trained = set(name for tab in tables for name, _, _ in tab)
        self._frozen = {k: np.array(a, np.float32) for k, a in weights.items() if k not in trained}   # upsampler=False
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        # a shard's row: every gradient buffer on the 16-byte grid (the vector paths of the combine and of Adam), the scalars last
        self.row_offsets, off = [], 0
        for p in self.p:
            self.row_offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.row_scalars, self.row_floats = off, off + ROW_SCALARS
        self._rows = None                 # the [S, row_floats] buffer of the last sharded step, kept for the next
        self.global_step = 0              # completed steps
        self.lr_t = None                  # the bias-corrected rate of the last step, as handed to the kernel (float32)
        self.lr_history = []              # the scheduled rate of every step

    def _update(self, flats):
        """grad_sumsq chained over the buffers and adam_ema_step on each; returns the global norm (0-d float64 device tensor)"""
        n, t = self.global_step, self.global_step + 1
        lr = scheduled_lr(self.lr, n)
        self.lr_history.append(lr)
        self.lr_t = float(np.float32(lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)))
        decay_t = min(self.ema_decay, (1.0 + n) / (10.0 + n))
        for i, g in enumerate(flats):
            grad_sumsq(g, self.sumsq, accumulate=i > 0)
        for p, g, m, v, e in zip(self.p, flats, self.m, self.v, self.ema):
            adam_ema_step(p, g, m, v, e, self.lr_t, self.beta1, self.beta2, self.eps, decay_t,
                          sumsq=self.sumsq if self.clip_norm is not None else None,
                          clip_norm=self.clip_norm if self.clip_norm is not None else 1.0)
        return self.sumsq.sqrt()[0]

    DEFER_NON_CONVERGENCE = False     # True: a shard that did not converge fails the step only after every shard has run

    def _plan(self, inputs, micro_batch, noise=None):
        """A step's cut, settled before anything is computed -- every refusal here is one all ranks share, so none of them
        leaves the others waiting in the exchange.  None: one shard, the unsharded path.  Otherwise (m, S, first shard, one
        past the last shard of this rank)."""
        if micro_batch is None and self.world == 1:
            return None
        who = type(self).__name__
        per_row = [(k, inputs[k]) for k in ROW_INPUTS if k in inputs] + ([('noise', noise)] if noise is not None else [])
        if 'mel' not in inputs:
            raise KeyError("{}.step: inputs lack 'mel'".format(who))
        B = int(inputs['mel'].shape[0])
        for k, v in per_row:
            if int(v.shape[0]) != B:
                raise ValueError('{}.step: {} has {} rows, mel has {}'.format(who, k, int(v.shape[0]), B))
        m = B if micro_batch is None else int(micro_batch)
        S, (lo, hi), _ = shard_plan(B, m, self.world, self.rank)
        return None if S == 1 else (m, S, lo, hi)

    def _sharded_step(self, inputs, plan, noise=None):
        """shards lo .. hi - 1 into their rows, the exchange, the combine, the update; returns (the shards' outputs, the
        step's dict: the combined scalars, 'log_probs' of this rank's rows where the model gives them, 'rows', 'grad_norm')"""
        from . import dist as wdist
        from .engine import grad_combine
        m, S, lo, hi = plan
        dev = self.eng.device
        if self._rows is None or int(self._rows.shape[0]) != S:
            self._rows = None             # let go of the old buffer first
            self._rows = torch.zeros(S, self.row_floats, dtype=torch.float32, device=dev)
        buf = self._rows
        outs, failed = [], []
        for j in range(lo, hi):
            rows = {k: inputs[k][j * m:(j + 1) * m] for k in ROW_INPUTS if k in inputs}
            try:
                out, flats = self._shard(rows, j, None if noise is None else noise[j * m:(j + 1) * m])
            except NotConverged as e:
                if not self.DEFER_NON_CONVERGENCE:
                    raise
                failed.append('shard {}: {}'.format(j, e))
                continue
            row = buf[j]
            for off, g in zip(self.row_offsets, flats):
                row[off:off + g.numel()].copy_(g)
            for i, key in enumerate(SCALAR_KEYS):         # a slot without its key stays at the zero it was created with
                if key in out:
                    row[self.row_scalars + i].copy_(out[key])
            outs.append(out)
        if failed:
            raise NotConverged('{}.step: {} of {} shards did not converge, nothing was updated; {}'.format(
                type(self).__name__, len(failed), hi - lo, '; '.join(failed)))
        with torch.cuda.device(dev):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.record_events else None
            if ev:
                ev[0].record()
            if self.world > 1:
                wdist.exchange_rows(buf, lo, hi)
            if ev:
                ev[1].record()
            grad_combine(buf, out=buf[0])
            if ev:
                ev[2].record()
                self.last_events = ev
        scalars = buf[0, self.row_scalars:].clone()           # row 0 is the next step's first row
        norm = self._update([buf[0, off:off + p.numel()] for off, p in zip(self.row_offsets, self.p)])
        self._repack(self.p)
        self.global_step += 1
        ret = {key: scalars[i] for i, key in enumerate(SCALAR_KEYS) if key in outs[0]}
        if 'log_probs' in outs[0]:
            ret['log_probs'] = torch.cat([o['log_probs'] for o in outs], dim=0)
        ret['rows'] = torch.arange(lo * m, hi * m, device=dev)
        ret['grad_norm'] = norm
        return outs, ret

    def weights(self, ema=False):
        """{tf name: numpy array in the TF shape} of every variable of the model: the weights, or with ema=True the shadow
        values under the plain names (what make_eval_model.py writes), for load_weights or an .npz for restore.  Variables that
        are not trained (the upsampler's with upsampler=False) come back as they were given."""
        out = {k: a.copy() for k, a in self._frozen.items()}
        for tab, buf in zip(self.tables, self.ema if ema else self.p):
            host = buf.cpu().numpy()
            for name, off, shape in tab:
                out[name] = host[off:off + int(np.prod(shape))].reshape(shape).copy()
        return out

    def use_ema(self):
        """Pack the shadow values into the handle, for generation after training (use_weights() puts the weights back)."""
        self._repack(self.ema)
        return self

    def use_weights(self):
        self._repack(self.p)
        return self

    def save(self, logdir):
        """Write model.ckpt-<global_step> into logdir as a TF V2 bundle with the keys tf.train.Saver writes for the
        reference's training graph -- '<var>', '<var>/Adam', '<var>/Adam_1', '<var>/ExponentialMovingAverage' for every
        trained variable, the plain name alone for a frozen one, 'global_step', 'beta1_power', 'beta2_power' -- and the
        `checkpoint` state file.  The eval CLIs load the directory as it is (shadows preferred); restore() continues from it.
        Returns the prefix.  In a data-parallel run every rank holds the same state: rank 0 alone writes, the others return
        the prefix it writes to."""
        if self.rank != 0:
            return os.path.join(logdir, 'model.ckpt-{:d}'.format(self.global_step))
        host = [[b.cpu().numpy() for b in bufs] for bufs in (self.p, self.m, self.v, self.ema)]
        trained = {}
        for i, tab in enumerate(self.tables):
            for name, off, shape in tab:
                n = int(np.prod(shape))
                trained[name] = tuple(h[i][off:off + n].reshape(shape) for h in host)
        return write_checkpoint(logdir, checkpoint_tensors(trained, self._frozen, self.global_step, self.beta1, self.beta2))

    def restore(self, prefix_or_logdir):
        """Refill the weights, both Adam moments, the shadows and global_step from a checkpoint save() wrote (a prefix, or a
        directory: its latest) and re-pack the handle with the weights.  The next step then has the bits of the run that
        wrote the checkpoint.  KeyError naming the first missing key, ValueError naming a key whose shape disagrees.  Frozen
        variables are the handle's: they are not reloaded."""
        from . import tf_bundle
        prefix = resolve_checkpoint(prefix_or_logdir)
        r = tf_bundle.BundleReader(prefix)
        if not r.has_tensor('global_step'):
            raise KeyError('checkpoint {} lacks global_step'.format(prefix))
        host = [[np.zeros(b.numel(), np.float32) for b in self.p] for _ in range(4)]
        for i, tab in enumerate(self.tables):
            for name, off, shape in tab:
                for h, suffix in zip(host, ('', ADAM_M, ADAM_V, wts.EMA)):
                    key = name + suffix
                    if not r.has_tensor(key):
                        raise KeyError('checkpoint {} lacks {}'.format(prefix, key))
                    if list(r.entries[key]['shape']) != list(shape):
                        raise ValueError('checkpoint {}: {} has shape {}, the model expects {}'.format(
                            prefix, key, list(r.entries[key]['shape']), list(shape)))
                    h[i][off:off + int(np.prod(shape))] = r.get_tensor(key).reshape(-1)
        for bufs, h in zip((self.p, self.m, self.v, self.ema), host):
            for b, a in zip(bufs, h):
                b.copy_(torch.from_numpy(a))
        self.global_step = int(r.get_tensor('global_step'))
        self.lr_t, self.lr_history = None, []
        self._repack(self.p)
        return self


class TeacherTrainer(_DeviceTrainer):
    """One teacher handle trained step after step.

    wavenet:  a loaded Wavenet (MoL or Gauss, no mu-law, no weight norm; a resize-conv upsampler needs upsampler=False).
    weights:  the dict it was loaded from -- the handle keeps no host copy, and the packs do not give the values back exactly.
    lr:       a float or a {step: lr} schedule keyed by the number of completed steps (scheduled_lr).
    clip_norm: None, or the bound of tf.clip_by_global_norm over all trained variables.
    upsampler: also train trans_conv_j/kernel and /bias; with False the upsampler keeps its weights.
    dropout:  apply the hparams' dropout_inputs / dropout_all (rate dropout_rate) in every step, as train_wavenet.py does
              (DESIGN.md 17); off by default.  Step k (k completed steps before it) draws its masks from the seed
              dropout_step_seed(dropout_seed, k), so a trainer built with global_step = n set continues the same sequence.
              feed_forward, calculate_loss and generation on the handle stay deterministic, like the reference's
              use_as_teacher graph.
    data_parallel: (keyword) True under an initialised torch.distributed group: the trainer computes its rank's shards of
              every step and all ranks keep the same state (_DeviceTrainer).
    step(batch, micro_batch=m) runs the step in B / m shards, shard j under the seed shard_seed(step seed, j); the result is
    a function of (B, m) and not of the number of ranks.

    Order inside a step (the reference's tf.group leaves it open): Adam first, with t = completed steps + 1; then the EMA of
    the UPDATED weights with num_updates = the number of steps completed BEFORE this one, i.e. the decay of step 1 is
    min(ema_decay, 1 / 10).  The shadows start equal to the weights."""

    def __init__(self, wavenet, weights, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.9999, clip_norm=None,
                 upsampler=True, dropout=False, dropout_seed=0):
        self.net = wavenet
        self.eng = eng = wavenet.engine
        self._init_optimiser(lr, beta1, beta2, eps, ema_decay, clip_norm)
        self.upsampler = bool(upsampler)
        self.dropout, self.dropout_seed = bool(dropout), int(dropout_seed)
        if self.dropout and not (wavenet.dropout_inputs or wavenet.dropout_all):
            raise ValueError('TeacherTrainer: dropout=True, but the hparams set neither dropout_inputs nor dropout_all')
        tables = [eng.teacher_grad_table()]
        if self.upsampler:
            tables.append(eng.deconv_grad_table(''))
        if not all(tables):
            raise ValueError('TeacherTrainer: this model has no weight gradients on the device (mu-law, ce, weight norm or '
                             'a resize-conv upsampler with upsampler=True)')
        sizes = [eng.teacher_grad_floats()] + ([eng.deconv_grad_floats('')] if self.upsampler else [])
        self._init_buffers(weights, tables, sizes)

    def _shard(self, inputs, j=0, noise=None):
        """(the call's dict, its flat gradients in table order) of shard j of the current step; j = 0 on the whole batch is
        the unsharded step"""
        seed = shard_seed(dropout_step_seed(self.dropout_seed, self.global_step), j) if self.dropout else None
        out = self.net.loss_and_weight_grads(inputs, upsampler=self.upsampler, dropout_seed=seed)
        flats = [out['flat_grads']]
        if self.upsampler:
            flats.append(out['flat_upsampler_grads'])
        return out, flats

    def _grads(self, inputs):
        return self._shard(inputs)

    def _repack(self, bufs):
        self.eng.teacher_set_weights(bufs[0], bufs[1] if self.upsampler else None)

    def step(self, inputs, micro_batch=None):
        """One training step on {'wav': [B,T], 'mel': [B,F,80]} -> {'loss': the loss BEFORE the update (the bits of
        calculate_loss(feed_forward(.)) under the weights in force at entry; with dropout those of
        loss_and_weight_grads(dropout_seed=dropout_step_seed(dropout_seed, global_step))), 'log_probs': [B,T], 'grad_norm':
        the global norm of the gradient before clipping}, all device tensors.

        micro_batch=m < B: the step in S = B / m shards (the class's notes).  Shard j is
        loss_and_weight_grads on rows [j m, (j + 1) m) under dropout_seed = shard_seed(dropout_step_seed(dropout_seed,
        global_step), j); 'loss' is the combine of the shards' losses (float32), 'log_probs' holds the rows this process
        computed, in shard order, and 'rows' names their indices in the batch.  None or m = B is the step above, bit for bit."""
        plan = self._plan(inputs, micro_batch)
        if plan is not None:
            return self._sharded_step(inputs, plan)[1]
        out, flats = self._shard(inputs)
        norm = self._update(flats)
        self._repack(self.p)
        self.global_step += 1
        return {'loss': out['loss'], 'log_probs': out['log_probs'], 'grad_norm': norm}


class StudentTrainer(_DeviceTrainer):
    """One student handle distilled step after step (train_parallel_wavenet.py's loop).

    pw:       a loaded ParallelWavenet with a teacher (logistic under a MoL teacher or Gauss under Gauss; no mu-law, no weight
              norm; width and deconv_width multiples of 64).  The teacher stays frozen.
    weights:  the dict the student was loaded from.
    lr, beta1, beta2, eps, ema_decay, clip_norm: as for TeacherTrainer.
    upsampler: also train the deconv stacks the student owns ('iaf_share', or 'iaf_k' per flow), as the reference's
              filter_update_variables keeps them; with use_teacher_deconv the encoding is the teacher's and no stack is trained.
    seed:     step k (k completed steps before it) runs loss_and_weight_grads(seed=seed + k): the student's draw (unless
              `noise` is handed to step) and the Monte-Carlo draws of the losses.  Shard j of a sharded step
              (step(batch, micro_batch=m)) runs under shard_seed(seed + k, j).
    data_parallel: (keyword) as for TeacherTrainer.

    Buffers: one (p, m, v, ema) set for the flows, laid out by Engine.iaf_grad_table(), and one per trained stack, laid out
    by Engine.deconv_grad_table(scope).  Order inside a step, the learning-rate schedule and the EMA decay are
    TeacherTrainer's."""

    def __init__(self, pw, weights, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.9999, clip_norm=None,
                 upsampler=True, seed=0):
        if getattr(pw, 'teacher', None) is None:
            raise ValueError('StudentTrainer needs a student with a teacher: ParallelWavenet(hparams, teacher=Wavenet(te_hparams))')
        self._init_student(pw, weights, lr, beta1, beta2, eps, ema_decay, clip_norm, upsampler)
        self.seed = int(seed)

    def _init_student(self, pw, weights, lr, beta1, beta2, eps, ema_decay, clip_norm, upsampler):
        """the optimiser and the buffers of the flows and of every trained stack (StudentMleTrainer's as well)"""
        who = type(self).__name__
        self.net = pw
        self.eng = eng = pw.engine
        self._init_optimiser(lr, beta1, beta2, eps, ema_decay, clip_norm)
        self.upsampler = bool(upsampler) and not getattr(pw, 'use_teacher_deconv', False)
        tables = [eng.iaf_grad_table()]
        if not tables[0]:
            raise ValueError('{}: this model has no weight gradients on the device (mu-law, weight norm, or a '
                             'width / deconv_width that is no multiple of 64)'.format(who))
        sizes = [eng.iaf_grad_floats()]
        self.scopes = list(eng.iaf_stack_scopes()) if self.upsampler else []
        for scope in self.scopes:
            tables.append(eng.deconv_grad_table(scope))
            sizes.append(eng.deconv_grad_floats(scope))
        if not all(tables):
            raise ValueError('{}: a deconv stack has no weight gradients on the device (a resize-conv upsampler needs '
                             'upsampler=False)'.format(who))
        self._init_buffers(weights, tables, sizes)

    def _repack(self, bufs):
        self.eng.iaf_set_weights(bufs[0], dict(zip(self.scopes, bufs[1:])))

    def _shard(self, inputs, j=0, noise=None):
        out = self.net.loss_and_weight_grads(inputs, seed=shard_seed(self.seed + self.global_step, j), noise=noise,
                                             upsampler=self.upsampler)
        return out, [out['flat_grads']] + [out['flat_upsampler_grads'][s] for s in self.scopes]

    def step(self, inputs, noise=None, micro_batch=None):
        """One training step on {'mel': [B,F,80], 'wav': [B,T'] (+ 'mel_rand')} -> calculate_loss's entries BEFORE the update
        (the bits of loss_and_weight_grads(inputs, seed=seed + global_step, noise=noise) under the weights in force at entry)
        plus 'grad_norm', the global norm of the gradient before clipping; all device tensors.

        micro_batch=m < B: the step in S = B / m shards (_DeviceTrainer's notes).  Shard j is
        loss_and_weight_grads on rows [j m, (j + 1) m) of the inputs (and of `noise`) under seed = shard_seed(seed +
        global_step, j); every entry of calculate_loss is the combine of the shards' (float32), and 'rows' names the rows this
        process computed.  None or m = B is the step above, bit for bit."""
        plan = self._plan(inputs, micro_batch, noise)
        if plan is not None:
            return self._sharded_step(inputs, plan, noise)[1]
        out, flats = self._shard(inputs, 0, noise)
        norm = self._update(flats)
        self._repack(self.p)
        self.global_step += 1
        ret = {k: v for k, v in out.items() if k not in ('grads', 'flat_grads', 'd_encoding', 'flat_upsampler_grads')}
        ret['grad_norm'] = norm
        return ret


class StudentMleTrainer(StudentTrainer):
    """One student handle trained by maximum likelihood on real audio: the loss is -mean log p(wav | mel) of
    ParallelWavenet.nll_and_weight_grads, and no teacher is needed -- ParallelWavenet(hparams) will do, and a teacher the
    student has is not used.  Also the likelihood fine-tuning of a distilled student.

    pw, weights, lr, beta1, beta2, eps, ema_decay, clip_norm, upsampler: as for StudentTrainer (no mu-law, no weight norm;
    width and deconv_width multiples of 64).  encode_tol: the tolerance of the encode's sweeps (README: 1e-5 for the shipped
    student); adjoint_tol: that of the adjoint's (None: Engine.ADJOINT_TOL).  max_sweeps: the bound of both, None for T.
    The buffers, the update, the re-pack, save() and restore() are StudentTrainer's; nothing is drawn, so there is no seed.
    step(batch, micro_batch=m) shards the step in one process; data_parallel=True is refused (a rank that did not converge
    could not tell the others before the exchange)."""

    def __init__(self, pw, weights, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.9999, clip_norm=None,
                 upsampler=True, encode_tol=1e-5, adjoint_tol=None, max_sweeps=None):
        for name, tol in (('encode_tol', encode_tol), ('adjoint_tol', adjoint_tol)):
            if tol is not None and not float(tol) >= 0.0:
                raise ValueError('StudentMleTrainer: {} must be >= 0, got {}'.format(name, tol))
        if encode_tol is None:
            raise ValueError('StudentMleTrainer: encode_tol must be >= 0, got None')
        if max_sweeps is not None and int(max_sweeps) < 1:
            raise ValueError('StudentMleTrainer: max_sweeps must be >= 1, got {}'.format(max_sweeps))
        if getattr(pw, 'use_mu_law', False):
            raise ValueError('StudentMleTrainer: mu-law students are not supported (their audio is not the flow\'s output x)')
        self._init_student(pw, weights, lr, beta1, beta2, eps, ema_decay, clip_norm, upsampler)
        self.encode_tol, self.adjoint_tol = float(encode_tol), None if adjoint_tol is None else float(adjoint_tol)
        self.max_sweeps = None if max_sweeps is None else int(max_sweeps)

    DATA_PARALLEL_REFUSAL = ('a rank whose encode or adjoint did not converge would have to tell the others through the '
                             'exchange; run the shards in one process (micro_batch=)')
    DEFER_NON_CONVERGENCE = True

    def _shard(self, inputs, j=0, noise=None):
        kw = {} if self.max_sweeps is None else {'max_sweeps': self.max_sweeps}
        out = self.net.nll_and_weight_grads(inputs, upsampler=self.upsampler, encode_tol=self.encode_tol,
                                            adjoint_tol=self.adjoint_tol, **kw)
        return out, [out['flat_grads']] + [out['flat_upsampler_grads'][s] for s in self.scopes]

    def step(self, inputs, micro_batch=None):
        """One training step on {'mel': [B,F,80], 'wav': [B,T']} -> {'loss': -mean log p BEFORE the update (the bits of
        nll_and_weight_grads under the weights in force at entry), 'log_probs', 'grad_norm': the global norm of the gradient
        before clipping, 'sweeps', 'adjoint_sweeps', 'converged'}.  Raises, with nothing updated, when the encode or the
        adjoint did not converge.

        micro_batch=m < B: the step in S = B / m shards (_DeviceTrainer's notes), shard j being
        nll_and_weight_grads on rows [j m, (j + 1) m).  'loss' is the combine of the shards' losses (float32), 'sweeps' and
        'adjoint_sweeps' the largest of any shard, 'converged' and 'log_probs' cover all rows, 'rows' names them.  Every
        shard runs; if one did not converge the step raises afterwards, with nothing updated.  None or m = B is the step
        above, bit for bit.  One process only: data_parallel=True is refused."""
        for k in ('mel', 'wav'):
            if k not in inputs:
                raise KeyError('StudentMleTrainer.step: inputs lack {!r}'.format(k))
        plan = self._plan(inputs, micro_batch)
        if plan is not None:
            outs, ret = self._sharded_step(inputs, plan)
            ret.update({'sweeps': max(o['sweeps'] for o in outs), 'adjoint_sweeps': max(o['adjoint_sweeps'] for o in outs),
                        'converged': torch.cat([o['converged'] for o in outs])})
            return ret
        out, flats = self._shard(inputs)
        norm = self._update(flats)
        self._repack(self.p)
        self.global_step += 1
        return {'loss': out['loss'], 'log_probs': out['log_probs'], 'grad_norm': norm, 'sweeps': out['sweeps'],
                'adjoint_sweeps': out['adjoint_sweeps'], 'converged': out['converged']}
