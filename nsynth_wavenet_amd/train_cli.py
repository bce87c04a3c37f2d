"""Shared body of the two training CLIs (train_wavenet.py, train_parallel_wavenet.py).

Keeps the reference's command-line surface (train_wavenet.py:182-202 / train_parallel_wavenet.py:230-252 there):
--config --train_path --logdir --log_root --total_batch_size --log --gpu_id, plus --teacher_dir for the student, and its
logdir convention: with --log_root a new directory log_root/<kind>-<time stamp> that gets a copy of the config json;
without it the run in --logdir continues from its single *.json and its latest checkpoint.  Added: --num_iters --seed
--save_interval_steps --save_interval_secs --log_every_n_steps --dropout/--no-dropout --clip_norm --micro_batch_size.

The loop is train.DeviceDataset.batch(global_step) -> trainer.step: the batch, the dropout masks and the student's draws
are functions of global_step, so a continued run repeats the bits of an uninterrupted one.  The host reads
the loss only every --log_every_n_steps steps.

Data parallel: under torch.distributed.run (WORLD_SIZE > 1) every process trains on the GPU LOCAL_RANK, the
step runs in total_batch_size / micro_batch_size shards spread over the ranks, and the run has the bits of the one-process
run with the same two sizes.  Rank 0 alone creates the run directory and writes train.log and the checkpoints.

Left out, each refused with a message: more than one id in --gpu_id (the reference's multi-clone deployment; several GPUs
are several processes under torch.distributed.run instead), the models
the trainers refuse (mu-law, ce, weight norm), data-dependent initialisation (weight norm only), TensorBoard summaries
(train.log carries the scalars).
"""
import glob
import json
import logging
import os
import shutil
import time
from argparse import ArgumentParser

import numpy as np

from .config import load_hparams

# wavenet.py:7-14 of the reference
DEFAULT_LR_SCHEDULE = {0: 2e-4, 90000: 4e-4 / 3, 120000: 6e-5, 150000: 4e-5, 180000: 2e-5, 210000: 6e-6, 240000: 2e-6}
KINDS = {'teacher': 'wavenet', 'student': 'parallel_wavenet'}


def build_parser(kind):
    p = ArgumentParser(description='Train the {} on one GPU.'.format(
        'WaveNet teacher' if kind == 'teacher' else 'Parallel-WaveNet student under a trained teacher'))
    p.add_argument('--config', required=False, help='Model configuration json (needed with --log_root).')
    p.add_argument('--train_path', required=True, help='TFRecord of the training utterances (written by build_dataset.py).')
    if kind == 'student':
        p.add_argument('--teacher_dir', required=True, help="The teacher's logdir: its single *.json and latest checkpoint.")
    p.add_argument('--logdir', default='/tmp/nsynth', help='The log directory of a run to continue.')
    p.add_argument('--log_root', default='', help='Start a new run in a fresh directory under this one.')
    p.add_argument('--total_batch_size', default=4, type=int, help='Utterance crops per step.')
    p.add_argument('--log', default='INFO', help='DEBUG, INFO, WARN, ERROR, or FATAL.')
    p.add_argument('--gpu_id', default='0', help='The GPU to train on (one id).')
    # not in the reference
    p.add_argument('--num_iters', default=None, type=int, help="Total number of steps; overrides the hparams' num_iters.")
    p.add_argument('--seed', default=0, type=int, help='Seed of the initial weights, the batches and every random draw.')
    p.add_argument('--save_interval_steps', default=0, type=int, help='Also save every this many steps (0: off).')
    p.add_argument('--save_interval_secs', default=3600, type=float, help='Save when this many seconds have passed.')
    p.add_argument('--log_every_n_steps', default=100, type=int, help='Read and log the loss every this many steps.')
    p.add_argument('--clip_norm', default=None, type=float, help='Bound of clip_by_global_norm (default: no clipping).')
    if kind == 'teacher':
        p.add_argument('--dropout', dest='dropout', action='store_true', default=None,
                       help="Apply the hparams' dropout_inputs / dropout_all (the default where the hparams set one).")
        p.add_argument('--no-dropout', dest='dropout', action='store_false', help='Train without dropout.')
    return p


def cli_parser(kind):
    """The parser the two scripts use: build_parser's single-GPU surface and the flag of the sharded step"""
    p = build_parser(kind)
    p.add_argument('--micro_batch_size', default=None, type=int,
                   help='Crops per gradient call: a step runs in total_batch_size / micro_batch_size shards, spread over the '
                        'processes of torch.distributed.run (default: total_batch_size / WORLD_SIZE, one shard per process).')
    return p


def single_json(directory, flag):
    jsons = sorted(glob.glob(os.path.join(directory, '*.json')))
    if len(jsons) != 1:
        raise RuntimeError('{} {} must hold exactly one *.json config, found {}'.format(flag, directory, len(jsons)))
    return jsons[0]


def check_gpu_id(gpu_id):
    ids = [s for s in str(gpu_id).split(',') if s.strip()]
    if len(ids) != 1:
        raise RuntimeError('--gpu_id {!r}: training runs on exactly one GPU; the multi-clone deployment of the reference '
                           '(several ids) and CPU training (no id) are not supported'.format(gpu_id))
    return ids[0].strip()


def resolve_micro_batch(args, world=None):
    """--micro_batch_size, or total_batch_size / WORLD_SIZE without the flag -- one shard per process, which for a single
    process is the unsharded step"""
    world = int(os.environ.get('WORLD_SIZE', '1')) if world is None else int(world)
    B = int(args.total_batch_size)
    if getattr(args, 'micro_batch_size', None) is not None:
        return int(args.micro_batch_size)
    if B % world != 0:
        raise RuntimeError('--total_batch_size {} does not split over {} processes; give --micro_batch_size'.format(B, world))
    return B // world


def resolve_run(args, kind, now=None):
    """(hparams dict, config json path, logdir, fresh): a new run under --log_root, else the run in --logdir"""
    if args.log_root:
        if args.config is None:
            raise RuntimeError('No config json specified: --log_root starts a new run and needs --config.')
        with open(args.config, 'rt') as f:
            hp = json.load(f)
        logdir = os.path.join(args.log_root, '{}-{}'.format(KINDS[kind], time.strftime('%Y%m%d-%H%M%S', time.localtime(now))))
        os.makedirs(logdir, exist_ok=True)
        shutil.copy(args.config, logdir)
        return hp, os.path.join(logdir, os.path.basename(args.config)), logdir, True
    logdir = args.logdir
    if not os.path.isdir(logdir):
        raise RuntimeError('--logdir {} is not a directory (start a new run with --log_root and --config)'.format(logdir))
    config_json = single_json(logdir, '--logdir')
    with open(config_json, 'rt') as f:
        hp = json.load(f)
    return hp, config_json, logdir, False


def resolve_num_iters(args, hp):
    n = args.num_iters if args.num_iters is not None else hp.get('num_iters')
    if n is None:
        raise RuntimeError("the number of steps is given neither by --num_iters nor by the config's \"num_iters\"")
    return int(n)


def lr_schedule(hp):
    """the hparams' lr_schedule ({step: lr}, json string keys, or [[step, lr], ...]) with int keys in the file's order;
    DEFAULT_LR_SCHEDULE without one"""
    sched = (hp if isinstance(hp, dict) else vars(hp)).get('lr_schedule', DEFAULT_LR_SCHEDULE)
    items = sched.items() if isinstance(sched, dict) else sched
    return {int(k): float(v) for k, v in items}


def init_from_teacher(weights, teacher_weights):
    """Every trans_conv_* / resize_conv_* variable of the student takes the teacher's value (the reference's
    _trans_conv_init_from_teacher: a student variable whose name ends with the teacher's).  Returns the names set."""
    done = []
    for name in weights:
        leaf = name.split('/', 1)[1] if '/' in name else name
        if leaf.startswith(('trans_conv_', 'resize_conv_')) and name.startswith('iaf') and leaf in teacher_weights:
            if np.shape(weights[name]) != np.shape(teacher_weights[leaf]):
                raise ValueError('{} has shape {}, the teacher\'s {} has {}'.format(
                    name, np.shape(weights[name]), leaf, np.shape(teacher_weights[leaf])))
            weights[name] = np.array(teacher_weights[leaf], np.float32)
            done.append(name)
    return done


class RunLog(object):
    """one line per logged step, to stdout and to <logdir>/train.log"""

    def __init__(self, logdir, enabled=True):
        self.path, self.enabled = os.path.join(logdir, 'train.log'), enabled

    def line(self, text):
        if not self.enabled:                  # a rank other than 0 of a data-parallel run
            return
        print(text, flush=True)
        with open(self.path, 'at') as f:
            f.write(text + '\n')


def _scalar(x):
    return float(x.detach().double().cpu()) if hasattr(x, 'detach') else float(x)


def train_loop(trainer, ds, args, logdir, num_iters, mel_rand=False, extra_keys=()):
    """ds.batch(global_step) -> trainer.step until num_iters; logs every log_every_n_steps, saves at the intervals and at the
    end.  Returns the number of steps run.  Every rank of a data-parallel run is handed the full batch of the step; rank 0
    alone reads the loss, logs and saves -- none of which is a collective, so the ranks need not agree on the clock."""
    import torch
    first = getattr(trainer, 'rank', 0) == 0
    log = RunLog(logdir, enabled=first)
    micro = resolve_micro_batch(args, getattr(trainer, 'world', 1))
    every = max(1, int(args.log_every_n_steps))
    last_save, t_mark, n_mark, ran = time.time(), time.time(), trainer.global_step, 0
    while trainer.global_step < num_iters:
        out = trainer.step(ds.batch(trainer.global_step, args.total_batch_size, mel_rand=mel_rand), micro_batch=micro)
        ran += 1
        step = trainer.global_step
        if first and (step % every == 0 or step == num_iters):
            vals = ['loss {:.17g}'.format(_scalar(out['loss']))]              # the host waits for the device here only
            now = time.time()
            vals.append('sec/step {:.4f}'.format((now - t_mark) / max(1, step - n_mark)))
            vals.append('lr {:.6g}'.format(trainer.lr_history[-1]))
            vals += ['{} {:.17g}'.format(k, _scalar(out[k])) for k in extra_keys if k in out]
            log.line('step {:d} {}'.format(step, ' '.join(vals)))
            t_mark, n_mark = now, step
        due = args.save_interval_steps and step % args.save_interval_steps == 0
        if first and (due or step == num_iters or (args.save_interval_secs and time.time() - last_save >= args.save_interval_secs)):
            log.line('saved {}'.format(trainer.save(logdir)))
            last_save = time.time()
    torch.cuda.synchronize()
    return ran


def resolve_run_on_ranks(args, kind, rank, world):
    """resolve_run for a data-parallel run: rank 0 alone creates the directory of a new run; the others learn it from rank 0
    and read the config copy in it"""
    import torch.distributed as td
    if not args.log_root or world == 1:
        return resolve_run(args, kind)
    if args.config is None or not os.path.isfile(args.config):      # on every rank, before the collective
        raise RuntimeError('No readable config json specified: --log_root starts a new run and needs --config.')
    found = [resolve_run(args, kind) if rank == 0 else None]
    td.broadcast_object_list(found, src=0)
    return found[0]


def _setup(args, kind):
    """-> (hparams, logdir, fresh, num_iters, data_parallel).  data_parallel: '' for one process, 'own' where this call
    created the process group (device LOCAL_RANK), 'given' where the caller had initialised torch.distributed already -- its
    group and its current device are then used as they are.  Arguments are checked before the process group exists, so a
    refusal ends every rank alike."""
    import torch.distributed as td
    from . import dist as wdist
    from .train import MAX_SHARDS
    gpu = check_gpu_id(args.gpu_id)
    rank, world, local = wdist.env_rank_world()
    micro = resolve_micro_batch(args, world)
    if micro < 1 or args.total_batch_size % micro != 0 or (args.total_batch_size // micro) % world != 0:
        raise RuntimeError('--total_batch_size {} in shards of --micro_batch_size {} does not spread evenly over {} '
                           'process(es)'.format(args.total_batch_size, micro, world))
    if args.total_batch_size // micro > MAX_SHARDS:
        raise RuntimeError('--total_batch_size {} in shards of --micro_batch_size {} are {} shards; a step takes at most {}'.format(
            args.total_batch_size, micro, args.total_batch_size // micro, MAX_SHARDS))
    dp = ''
    if world > 1:
        import torch
        dp = 'given' if td.is_available() and td.is_initialized() else 'own'
        if dp == 'own':
            wdist.init_process_group(timeout_s=wdist.TRAIN_TIMEOUT_S)
            torch.cuda.set_device(local)            # LOCAL_RANK: --gpu_id does not pin HIP_VISIBLE_DEVICES
    else:
        os.environ.setdefault('HIP_VISIBLE_DEVICES', gpu)
    logging.basicConfig(level=getattr(logging, {'WARN': 'WARNING', 'FATAL': 'CRITICAL'}.get(str(args.log).upper(), str(args.log).upper()),
                                      logging.INFO))
    hp, config_json, logdir, fresh = resolve_run_on_ranks(args, kind, rank, world)
    num_iters = resolve_num_iters(args, hp)
    if rank == 0:
        logging.info('%s, using config from %s, saving to %s', 'new run' if fresh else 'continue running', config_json, logdir)
    return load_hparams(hp), logdir, fresh, num_iters, dp


def _finish(data_parallel):
    """the ranks leave together: rank 0's last save is on disk before any process goes on; a group _setup created ends here"""
    if data_parallel:
        import torch
        import torch.distributed as td
        td.barrier(**({'device_ids': [torch.cuda.current_device()]} if td.get_backend() == 'nccl' else {}))
        if data_parallel == 'own':
            td.destroy_process_group()


def run_teacher(args):
    from . import train, weights as wts
    from .wavenet.wavenet import Wavenet
    hp, logdir, fresh, num_iters, dp = _setup(args, 'teacher')
    ckpt = None if fresh else wts.latest_checkpoint(logdir)
    w = train.checkpoint_weights(ckpt, hp, 'teacher') if ckpt else wts.synthetic_weights(hp, 'teacher', seed=args.seed, init='tf')
    net = Wavenet(hp).load_weights(w)
    dropout = args.dropout if args.dropout is not None else bool(net.dropout_inputs or net.dropout_all)
    trainer = train.TeacherTrainer(net, w, lr=lr_schedule(hp), clip_norm=args.clip_norm, dropout=dropout, dropout_seed=args.seed,
                                   data_parallel=dp)
    if ckpt:
        trainer.restore(ckpt)
    ds = train.DeviceDataset.from_tfrecord(os.path.abspath(os.path.expanduser(args.train_path)), hp.wave_length, seed=args.seed)
    train_loop(trainer, ds, args, logdir, num_iters)
    _finish(dp)
    return logdir


def run_student(args):
    from . import train, weights as wts
    from .cli import resolve_model
    from .wavenet.parallel_wavenet import ParallelWavenet
    from .wavenet.wavenet import Wavenet
    hp, logdir, fresh, num_iters, dp = _setup(args, 'student')
    te_hp, te_ckpt = resolve_model(os.path.abspath(os.path.expanduser(args.teacher_dir)))
    te_w = wts.load_checkpoint(te_ckpt, te_hp, 'teacher')                       # the shadows, as the reference restores them
    teacher = Wavenet(te_hp).load_weights(te_w)
    ckpt = None if fresh else wts.latest_checkpoint(logdir)
    if ckpt:
        w = train.checkpoint_weights(ckpt, hp, 'student')
    else:
        w = wts.synthetic_weights(hp, 'student', seed=args.seed, init='tf')
        logging.info('upsampler initialised from the teacher: %s', ', '.join(init_from_teacher(w, te_w)))
    pw = ParallelWavenet(hp, teacher=teacher).load_weights(w)
    trainer = train.StudentTrainer(pw, w, lr=lr_schedule(hp), clip_norm=args.clip_norm, seed=args.seed, data_parallel=dp)
    if ckpt:
        trainer.restore(ckpt)
    ds = train.DeviceDataset.from_tfrecord(os.path.abspath(os.path.expanduser(args.train_path)), hp.wave_length, seed=args.seed)
    mel_rand = pw.loss_type == 'logistic' and float(getattr(hp, 'contrastive_loss_factor', 0.0)) > 0.0
    train_loop(trainer, ds, args, logdir, num_iters, mel_rand=mel_rand,
               extra_keys=('kl_loss', 'H_Ps', 'H_Ps_Pt', 'power_loss', 'contrastive_loss'))
    _finish(dp)
    return logdir


def main(kind, argv=None):
    args = cli_parser(kind).parse_args(argv)
    return (run_teacher if kind == 'teacher' else run_student)(args)
