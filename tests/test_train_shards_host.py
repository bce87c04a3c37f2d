"""Host-side tests of the sharded training step: the numpy twin of wn_grad_combine against float64, the
shard seeds, the cut of a batch into shards and ranks with its refusals, --micro_batch_size, the declaration and the
binding of wn_grad_combine, the trainers' data_parallel keyword, and the row exchange between two gloo processes."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from nsynth_wavenet_amd import _lib, train, train_cli
from nsynth_wavenet_amd import dist as wdist


@pytest.mark.parametrize('S', [1, 2, 3, 8, 64])
def test_combine_np_against_float64(S):
    """|combine_np - float64 mean| <= S 2^-24 sum_j |r_j| per element.  (With u = 2^-24 the left-to-right float32 sum errs by
    at most about (S - 1) u sum |r_j|, the rounded 1 / S and the product add 2 u |sum|, and the division by S shrinks both:
    the bound has room to spare for every S >= 2, and S = 1 is exact.)"""
    rs = np.random.RandomState(100 + S)
    rows = (rs.standard_normal([S, 4099]) * np.exp(rs.uniform(-6, 6, [S, 1]))).astype(np.float32)
    got = train.combine_np(list(rows))
    assert got.dtype == np.float32 and got.shape == (4099,)
    want = rows.astype(np.float64).sum(axis=0) / S
    bound = S * 2.0 ** -24 * np.abs(rows.astype(np.float64)).sum(axis=0)
    err = np.abs(got.astype(np.float64) - want)
    print('S', S, 'max err / bound', float((err / bound).max()))
    assert (err <= bound).all()
    # the order is left to right: the twin is the explicit loop
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = np.float32(acc + r)
    assert np.array_equal(got, acc * (np.float32(1) / np.float32(S)))
    assert np.array_equal(train.combine_np([rows[0]]), rows[0])                   # S = 1: a copy times 1
    with pytest.raises(ValueError, match='takes 1 to 64'):
        train.combine_np([rows[0]] * 65)


def test_shard_seed():
    for s in (0, 1, 12345, 2 ** 63 + 5, 2 ** 64 - 1):
        assert train.shard_seed(s, 0) == s
        assert all(0 <= train.shard_seed(s, j) < 2 ** 64 for j in range(64))
        assert train.shard_seed(s, 5) == train.shard_seed(s, 5)
    # distinct over the shards of 64 consecutive student steps (seed + k) ...
    for s in (0, 7, 2 ** 64 - 70):
        vals = [train.shard_seed(s + k, j) for k in range(64) for j in range(64)]
        assert len(set(vals)) == 64 * 64
        assert set(vals[0::64]) == set(s + k for k in range(64))                   # shard 0 is the step's own seed
    # ... and of 64 consecutive teacher steps (dropout_step_seed)
    vals = [train.shard_seed(train.dropout_step_seed(3, k), j) for k in range(64) for j in range(64)]
    assert len(set(vals)) == 64 * 64
    # a hash mix, not seed + j
    assert train.shard_seed(10, 1) != 11 and train.shard_seed(10, 2) - train.shard_seed(10, 1) != 1
    with pytest.raises(ValueError, match='negative'):
        train.shard_seed(0, -1)


def test_shard_plan_and_its_refusals():
    assert [train.shard_plan(8, 1, 8, r) for r in (0, 3, 7)] == [(8, (0, 1), (0, 1)), (8, (3, 4), (3, 4)), (8, (7, 8), (7, 8))]
    assert [train.shard_plan(8, 2, 2, r) for r in (0, 1)] == [(4, (0, 2), (0, 4)), (4, (2, 4), (4, 8))]
    assert train.shard_plan(4, 4, 1, 0) == (1, (0, 1), (0, 4))
    assert train.shard_plan(64, 1) == (64, (0, 64), (0, 64))
    with pytest.raises(ValueError, match=r'B = 8 rows does not split into micro-batches of m = 3: B % m must be 0'):
        train.shard_plan(8, 3)
    with pytest.raises(ValueError, match=r'B = 8 rows in micro-batches of m = 2 are S = 4 shards, which W = 3 ranks do not share '
                                         r'evenly: S % W must be 0'):
        train.shard_plan(8, 2, 3, 0)
    with pytest.raises(ValueError, match=r'S = 65 shards; a step takes at most 64'):
        train.shard_plan(65, 1)
    with pytest.raises(ValueError, match='B % m must be 0'):
        train.shard_plan(8, 0)


def test_micro_batch_size_flag(monkeypatch):
    for kind, extra in (('teacher', []), ('student', ['--teacher_dir', 't'])):
        p = train_cli.cli_parser(kind)
        a = p.parse_args(['--train_path', 'x', '--total_batch_size', '8'] + extra)
        assert a.micro_batch_size is None
        monkeypatch.delenv('WORLD_SIZE', raising=False)
        assert train_cli.resolve_micro_batch(a) == 8                               # one process: the unsharded step
        monkeypatch.setenv('WORLD_SIZE', '4')
        assert train_cli.resolve_micro_batch(a) == 2                               # total_batch_size / WORLD_SIZE
        assert train_cli.resolve_micro_batch(a, world=8) == 1
        with pytest.raises(RuntimeError, match='does not split over 3 processes'):
            train_cli.resolve_micro_batch(a, world=3)
        b = p.parse_args(['--train_path', 'x', '--total_batch_size', '8', '--micro_batch_size', '1'] + extra)
        assert b.micro_batch_size == 1 and train_cli.resolve_micro_batch(b) == 1


def test_grad_combine_is_declared_and_bound_alike():
    lib = _lib.load()
    assert 'wn_grad_combine' in _lib.SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'wnhip.h')).read()
    m = re.search(r'^WN_API int wn_grad_combine\s*\(([^;]*)\);', header, re.M | re.S)
    assert m, 'wn_grad_combine is not declared in include/wnhip.h'
    args = [a.strip() for a in m.group(1).split(',')]
    assert args == ['const float* rows', 'size_t n', 'size_t row_stride', 'int S', 'float* out', 'void* stream']
    assert len(lib.wn_grad_combine.argtypes) == 6
    # the argument checks need no device: they refuse before the launch
    for n, stride, S in ((0, 4, 1), (4, 4, 0), (4, 4, 65), (4, 3, 2)):
        assert lib.wn_grad_combine(16, n, stride, S, 32, None) == -22


class _StubEngine(object):
    device = 'cpu'

    def iaf_grad_table(self):
        return [('iaf_1/start_conv/W', 0, (1, 3, 1, 64))]

    def iaf_grad_floats(self):
        return 0

    def iaf_stack_scopes(self):
        return []


class _StubStudent(object):
    use_teacher_deconv = False
    use_mu_law = False
    teacher = object()
    engine = _StubEngine()


def test_data_parallel_keyword():
    assert not dist.is_initialized()
    with pytest.raises(ValueError, match='StudentTrainer: data_parallel=True needs an initialised torch.distributed process group'):
        train.StudentTrainer(_StubStudent(), {}, data_parallel=True)
    with pytest.raises(ValueError, match='TeacherTrainer: data_parallel=True needs an initialised'):
        train.TeacherTrainer(None, {}, data_parallel=True)
    with pytest.raises(ValueError, match='StudentMleTrainer: data_parallel=True is not supported'):
        train.StudentMleTrainer(_StubStudent(), {}, data_parallel=True)
    with pytest.raises(KeyError):                     # data_parallel=False goes on to the (missing) weights, as before
        train.StudentTrainer(_StubStudent(), {}, data_parallel=False)
    tr = object.__new__(train.TeacherTrainer)
    assert (tr.data_parallel, tr.world, tr.rank) == (False, 1, 0)


def test_plan_validates_before_any_shard():
    tr = object.__new__(train.TeacherTrainer)
    mel, wav = np.zeros([4, 9, 80], np.float32), np.zeros([4, 1600], np.float32)
    assert tr._plan({'mel': mel, 'wav': wav}, None) is None
    assert tr._plan({'mel': mel, 'wav': wav}, 4) is None                           # m = B: the unsharded step
    assert tr._plan({'mel': mel, 'wav': wav}, 1) == (1, 4, 0, 4)
    assert tr._plan({'mel': mel, 'wav': wav}, 2) == (2, 2, 0, 2)
    with pytest.raises(ValueError, match='wav has 3 rows, mel has 4'):
        tr._plan({'mel': mel, 'wav': wav[:3]}, 2)
    with pytest.raises(ValueError, match='noise has 2 rows, mel has 4'):
        tr._plan({'mel': mel, 'wav': wav}, 2, noise=wav[:2])
    with pytest.raises(ValueError, match='B % m must be 0'):
        tr._plan({'mel': mel, 'wav': wav}, 3)
    tr.world, tr.rank = 2, 1                                                       # a rank of two
    assert tr._plan({'mel': mel, 'wav': wav}, 1) == (1, 4, 2, 4)
    with pytest.raises(ValueError, match=r'B = 4 rows in micro-batches of m = 4 are S = 1 shards, which W = 2 ranks'):
        tr._plan({'mel': mel, 'wav': wav}, None)


def test_mle_step_defers_non_convergence_until_every_shard_ran():
    """on a stub: a shard that raises engine.NotConverged is noted and the next one still runs; the step then raises with
    nothing updated (the raise comes before the exchange, the combine and the update).  Any other error ends the step at once."""
    from nsynth_wavenet_amd.engine import NotConverged
    assert issubclass(NotConverged, RuntimeError)
    tr = object.__new__(train.StudentMleTrainer)
    tr.eng = _StubEngine()
    tr.p, tr.row_offsets, tr.row_scalars, tr.row_floats, tr._rows, tr.global_step = [torch.zeros(4)], [0], 4, 12, None, 0
    tr._update = tr._repack = lambda *a: pytest.fail('the step went on to the update')
    ran = []

    def shard(rows, j, noise=None):
        ran.append(j)
        if j in fail:
            raise fail[j]
        return {'loss': torch.tensor(1.0)}, [torch.ones(4)]
    tr._shard = shard
    inputs = {'mel': np.zeros([4, 9, 80], np.float32), 'wav': np.zeros([4, 1800], np.float32)}
    fail = {0: NotConverged('the inverse did not converge in 1 sweeps')}
    with pytest.raises(NotConverged, match=r'StudentMleTrainer.step: 1 of 2 shards did not converge, nothing was updated; shard 0: the inverse'):
        tr.step(inputs, micro_batch=2)
    assert ran == [0, 1] and tr.global_step == 0
    ran[:] = []
    fail = {0: RuntimeError('did not converge, says another error')}              # the type decides, not the words
    with pytest.raises(RuntimeError, match='says another error'):
        tr.step(inputs, micro_batch=2)
    assert ran == [0]
    # the distilled student does not defer: its calls have nothing that may fail to converge
    assert train.StudentTrainer.DEFER_NON_CONVERGENCE is False and train.StudentMleTrainer.DEFER_NON_CONVERGENCE is True


def _exchange_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    wdist.init_process_group('gloo', timeout_s=120)
    S, n = 4, 37
    _, (lo, hi), _ = train.shard_plan(S, 1, world, rank)
    buf = torch.full([S, n], -1.0)                     # what another rank owns is junk before the exchange
    for j in range(lo, hi):
        buf[j] = torch.arange(n, dtype=torch.float32) + 1000.0 * j
    wdist.exchange_rows(buf, lo, hi)
    bad = None
    try:
        wdist.exchange_rows(buf, 0, S)                 # not this rank's share: refused on both ranks alike, before the collective
    except ValueError as e:
        bad = str(e)
    q.put((rank, buf.numpy().tobytes(), bad))
    dist.barrier()
    dist.destroy_process_group()


def test_row_exchange_between_two_gloo_processes():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_exchange_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = {r: (b, bad) for r, b, bad in (q.get(timeout=180) for _ in procs)}
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    want = (np.arange(37, dtype=np.float32)[None, :] + 1000.0 * np.arange(4, dtype=np.float32)[:, None]).astype(np.float32)
    assert res[0][0] == res[1][0] == want.tobytes()
    assert all('are not the share of rank' in res[r][1] for r in (0, 1))
