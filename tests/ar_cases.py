"""Cases of the autoregressive (fastgen) step tests: tests/test_gpu_ar_heads.py (GPU), tests/test_ar_oracle.py (CPU, holds
the references of those tests inside their own conditions) and the sampler parity rule tests/test_gpu_ar.py shares with them.

Nothing here comes from the code under test: geometries are chosen from the layout cases of csrc/wn_ar.hip, bars are the
project's existing ones (K1: 2e-5 max(1, max |ref|); sampler parity: the margins of test_golden_ar), and every statistical
bound is five standard errors of the statistic under the law the fixed network output defines, computed from N.
"""
import functools
import math

import numpy as np

from conftest import load_json
from oracle import wavenet_np as O

# ---------------------------------------------------------------------------------------------------------------------
# 1. geometry x head x batch matrix of the teacher-forced step outputs (K1)
# ---------------------------------------------------------------------------------------------------------------------
K1_BAR = 2e-5                      # max |out - ref| <= K1_BAR * max(1, max |ref|): test_golden_ar's and the batched test's bar
TN = 80                            # multiple of 16 (full-sequence teacher); every ring (2 d + 1 <= 33 slots) wraps at least twice
ROWS = 33                          # utterances of a case; a batch of B takes the first B
BATCHES = (1, 3, 4, 17, 33)        # default policy: GEMV for 1 and 3, padded batches of 16, 32 and 64
GEMV_BATCH = 5                     # ... and the GEMV step with its batch walked in two chunks (WN_AR_MODE=gemv)
# Rows of a batch are bit-equal to the same rows of another batch only where both run the same step form.  Of BATCHES no two
# batched sizes share a form (4 -> 16 columns, 17 -> 32, 33 -> 64; 17 against 4 is ACROSS forms and not asserted), so the pairs
# are: the GEMV step at 1, 3 and 5 (forced), and each of 4 / 17 against the full padded batch of its own form (16 / 32).
SAME_FORM_PAIRS = ((1, 3), (4, 16), (17, 32))

# smallest shapes wn_create accepts (width, skip % 64, gate % 128) that give the batched gate GEMM, K = 3 W + Cd + G/2 in
# slabs of 256, its layout cases
GEOMETRIES = {
    # K 512: two whole slabs, the control (the first layer, K = 3 W + Cd = 448, already ends in a slab of 192)
    'A': dict(width=128, double_gate_width=False, skip_width=64, deconv_width=64),
    # K 320: ragged second slab of 64, skip != width, doubled gate (G 128, H 64) on the tuned tiles
    'B': dict(width=64, double_gate_width=True, skip_width=128, deconv_width=64),
    # K 896: four slabs, the last half full; G 384 = 24 gate row blocks, W + S = 256
    'C': dict(width=192, double_gate_width=True, skip_width=64, deconv_width=128),
}
SLAB_K = {'A': 512, 'B': 320, 'C': 896}
STACK = dict(num_layers=7, num_stages=5)       # dilations 1 2 4 8 16 1 2: the cycle ends inside the stack

HEADS = {
    'mol10': ('wavenet_mol.json', dict(mol_mix=10)),            # 30 output rows: a ragged 16-row block
    'mol1': ('wavenet_mol.json', dict(mol_mix=1)),              # 3 rows
    'mol64': ('wavenet_mol.json', dict(mol_mix=64)),            # 192 rows, 65 randoms per step
    'ce': ('wavenet_ce.json', dict(use_mu_law=True)),           # 256 rows, mu-law input encoding
    'gauss': ('wavenet_gauss.json', dict()),                    # 2 rows inside one 16-row block
}
# every geometry: mol10, ce, gauss; every head on at least two geometries
MATRIX = [('A', 'mol10'), ('A', 'ce'), ('A', 'gauss'), ('A', 'mol1'),
          ('B', 'mol10'), ('B', 'ce'), ('B', 'gauss'), ('B', 'mol64'),
          ('C', 'mol10'), ('C', 'ce'), ('C', 'gauss'), ('C', 'mol1'), ('C', 'mol64')]
MATRIX_IDS = ['{}-{}'.format(g, h) for g, h in MATRIX]


def config(geom, head):
    base, patch = HEADS[head]
    cfgd = dict(load_json(base), **STACK)
    cfgd.update(GEOMETRIES[geom])
    cfgd.update(patch)
    return cfgd


def padded_batch(B, gemv=False):
    """The step form wn_ar.hip documents for a batch: 0 = GEMV step, else the padded batch of the MFMA step."""
    if gemv or B < 4:
        return 0
    return 16 if B <= 16 else 32 if B <= 32 else (B + 63) // 64 * 64


MU_LAW_MARGIN = 1e-3


def forced_signal(rs, shape, hp):
    """Teacher-forcing samples in (-1, 1).  With mu-law the network input is floor(128 f(x)) / 128 (utils.py:72-87): a sample
    whose 128 f(x) sits within float32 rounding of an integer would encode one step apart in float32 and float64 and say
    nothing about the kernels.  128 f(x) <= 128 carries a few float32 ulps of log() error, < 1e-4; samples closer than
    MU_LAW_MARGIN = 1e-3 to an integer are redrawn (about 0.2 % of them)."""
    f = rs.uniform(-1, 1, shape).astype(np.float32)
    if hp.use_mu_law:
        for _ in range(16):
            y = np.sign(f) * np.log1p(255.0 * np.abs(f.astype(np.float64))) / np.log(256.0) * 128.0
            bad = np.abs(y - np.round(y)) < MU_LAW_MARGIN
            if not bad.any():
                break
            f[bad] = rs.uniform(-1, 1, int(bad.sum())).astype(np.float32)
        assert not bad.any()
    return f


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def case(geom, head):
    """(cfgd, hp, weights, enc [ROWS, TN, Cd], forced [ROWS, TN]) of one matrix case; the upsampler is left out (enc random)."""
    cfgd = config(geom, head)
    hp = O.HP(cfgd)
    seed = 1000 + 17 * MATRIX.index((geom, head))
    w = O.synth_weights(hp, 'teacher', seed=seed, init='unit')
    rs = np.random.RandomState(seed + 1)
    enc = (rs.standard_normal([ROWS, TN, hp.deconv_width]) * 0.5).astype(np.float32)
    forced = forced_signal(rs, [ROWS, TN], hp)
    _freeze(enc, forced)
    return cfgd, hp, w, enc, forced


@functools.lru_cache(maxsize=None)
def k1_reference(geom, head):
    """float64 full-sequence teacher on the case's ROWS utterances (computed once, read-only) and the K1 bar in absolute units."""
    _, hp, w, enc, forced = case(geom, head)
    ref = O.teacher_feed_forward(O.encode_signal(forced, hp, np.float64), enc.astype(np.float64), w, hp, np.float64)
    _freeze(ref)
    return ref, K1_BAR * max(1.0, float(np.abs(ref).max()))


def n_rand(hp):
    return hp.mol_mix + 1 if hp.loss_type == 'mol' else 1


def free_run_randoms(hp, Tn, B, seed):
    """Injected randoms [Tn, B, n_rand] of a free run: uniforms in (1e-5, 1 - 1e-5) (mol), N(0, 1) (gauss), [0, 1) (ce)."""
    rs = np.random.RandomState(seed)
    if hp.loss_type == 'gauss':
        return rs.standard_normal([Tn, B, 1]).astype(np.float32)
    if hp.loss_type == 'ce':
        return rs.uniform(0, 1, [Tn, B, 1]).astype(np.float32).clip(0, np.nextafter(np.float32(1), np.float32(0)))
    return rs.uniform(1e-5, 1 - 1e-5, [Tn, B, n_rand(hp)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the sampler parity rule (moved here from test_golden_ar: one copy for both GPU files and the CPU test)
# ---------------------------------------------------------------------------------------------------------------------
def sampler_parity(hp, out_params, rnd, idx):
    """Integer parity of the sampling head (loss_func.py:140-206) GIVEN the network output `out_params` [B, Tn, ow] the indices
    `idx` [B, Tn] were drawn from and the injected randoms `rnd` [Tn, B, n_rand]: against float64 arithmetic the index may
    differ by ONE step, and only where the pre-floor() quantity sits within float32 rounding of a decision boundary.
    Returns dict(d, margin, gap [B, Tn], n_flip, n_bad)."""
    B, Tn = idx.shape
    Q = O.quant_chann_of(hp)
    mol = hp.loss_type == 'mol'
    D = np.zeros([B, Tn], np.int64)
    M = np.zeros([B, Tn])
    G = np.full([B, Tn], np.inf)
    n_bad = n_flip = 0
    for t in range(Tn):
        i64, margin, gap = O.sample_margin(out_params[:, t], rnd[t], hp)
        d = idx[:, t].astype(np.int64) - i64
        flip = d != 0
        n_flip += int(flip.sum())
        if hp.loss_type == 'ce':
            ok = (np.abs(d) <= 1) & (~flip | (margin <= 2e-5))     # 256 fp32 running sums: ~1.5e-5 of the mass
        else:
            # |x| <= 1 in fp32 -> x*Q/2 carries <= ~4e-3 index units of rounding at Q = 65536 (libm exp/log 1-2 ulp)
            tol = 0.02 if Q == 65536 else 1e-3
            ok = (np.abs(d) <= 1) & (~flip | (margin <= tol))
            if mol:     # a different mixture component only where the two best scores tie within fp32 noise
                ok |= gap <= 1e-5
                G[:, t] = gap
        n_bad += int((~ok).sum())
        D[:, t], M[:, t] = d, margin
    return dict(d=D, margin=M, gap=G, n_flip=n_flip, n_bad=n_bad)


def assert_sampler_parity(tag, hp, out_params, rnd, idx):
    """The rule as test_golden_ar asserts it; returns the number of one-step differences at a boundary."""
    B, Tn = idx.shape
    p = sampler_parity(hp, out_params, rnd, idx)
    print('{}: sampler index vs float64: {} of {} differ by one step at a boundary, {} unexplained'.format(
        tag, p['n_flip'], B * Tn, p['n_bad']))
    assert p['n_bad'] == 0
    assert p['n_flip'] <= max(2, B * Tn // 20)
    return p['n_flip']


def dequant(idx, hp):
    """fastgen.py:163-167 in float32: the audio fed back for an index."""
    if hp.use_mu_law:
        return O.inv_mu_law(idx, dtype=np.float32)
    return O.inv_cast_quantize(idx, O.quant_chann_of(hp), np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. sampler edges on a fixed network output
# ---------------------------------------------------------------------------------------------------------------------
EDGE_GEOM = 'A'
EDGE_HEADS = {'mol': 'mol10', 'gauss': 'gauss', 'ce': 'ce'}
EDGE_BATCHES = (2, 16)              # GEMV layout [b][o] and the batched step's [o][NB]
EDGE_TN = 32


def fixed_output_weights(hp, row, seed=77):
    """Unit-init teacher whose out2/W is zero: the network output is out2/biases = `row` at every step and batch element,
    whatever is fed back (0 * z + b is exact in any arithmetic as long as z is finite)."""
    w = O.synth_weights(hp, 'teacher', seed=seed, init='unit')
    row = np.asarray(row, np.float32)
    assert row.shape == w['out2/biases'].shape
    w['out2/W'] = np.zeros_like(w['out2/W'])
    w['out2/biases'] = row
    return w


def sampler_facts(hp, row, rnd):
    """float64 internals of the sampler (loss_func.py:140-206) on ONE output row and randoms [..., n_rand]: what the
    'edge is reached' assertions read.  mol: k, ls_raw, x_pre (before the clip), x_unclamped (log-scale not clamped), gap;
    gauss: ls_raw, x_pre, x_unclamped; ce: e (softmax numerators), k."""
    row = np.asarray(row, np.float64)
    rnd = np.asarray(rnd, np.float64)
    if hp.loss_type == 'mol':
        M = hp.mol_mix
        sel = row[:M] - np.log(-np.log(rnd[..., :M]))
        k = np.argmax(sel, axis=-1)
        srt = np.sort(sel, axis=-1)
        u = rnd[..., M]
        lg = np.log(u) - np.log(1.0 - u)
        ls_raw = row[2 * M + k]
        return dict(k=k, ls_raw=ls_raw, gap=srt[..., -1] - srt[..., -2] if M > 1 else None,
                    x_pre=row[M + k] + np.exp(np.clip(ls_raw, -7.0, 7.0)) * lg, x_unclamped=row[M + k] + np.exp(ls_raw) * lg)
    if hp.loss_type == 'gauss':
        z = rnd[..., 0]
        return dict(ls_raw=row[1], x_pre=row[0] + np.exp(max(row[1], -7.0)) * z, x_unclamped=row[0] + np.exp(row[1]) * z)
    e = np.exp(row - row.max())
    cdf = np.cumsum(e)
    thr = rnd[..., 0] * cdf[-1]
    return dict(e=e, k=np.minimum((cdf <= thr[..., None]).sum(axis=-1), row.size - 1))


F32_BELOW_1 = np.nextafter(np.float32(1), np.float32(0))
U_LO, U_HI = np.float32(1e-5), np.float32(1 - 1e-5)


def _index(x, Q):
    return np.floor(np.clip(x, -1.0, 1.0 - 2.0 / Q) * (Q / 2.0)).astype(np.int64)


def _mol_edges(hp, B):
    M, Tn, Q = hp.mol_mix, EDGE_TN, 65536
    rs = np.random.RandomState(11)
    uni = lambda: rs.uniform(1e-5, 1 - 1e-5, [Tn, B, M + 1]).astype(np.float32)
    logits = rs.uniform(-1, 1, M)
    means = rs.uniform(-0.5, 0.5, M)
    out = []

    def low(f, rnd):        # held at -7: with e^-9 the draws would land elsewhere
        assert np.all(f['ls_raw'] < -7.0) and np.all(np.abs(f['x_pre']) < 0.9)
        assert (_index(f['x_unclamped'], Q) != _index(f['x_pre'], Q)).mean() > 0.5
    out.append(('log_scale_-9', np.r_[logits, means, np.full(M, -9.0)], uni(), low, False))

    def high(f, rnd):       # held at +7: every draw leaves [-1, 1) and both ends occur
        assert np.all(f['ls_raw'] > 7.0) and np.all(np.abs(f['x_pre']) > 2.0)
        assert (f['x_pre'] < 0).any() and (f['x_pre'] > 0).any()
    r = uni()
    r[..., M] = np.where(np.abs(r[..., M] - 0.5) < 0.01, np.float32(0.3), r[..., M])   # |logistic| >= 0.04: e^7 * 0.04 = 44
    out.append(('log_scale_+9', np.r_[logits, means, np.full(M, 9.0)], r, high, True))

    def far(f, rnd):        # means outside [-1, 1): clipped at both ends
        assert np.all(np.abs(f['x_pre']) > 1.2) and (f['x_pre'] < 0).any() and (f['x_pre'] > 0).any()
    out.append(('means_+-1.5', np.r_[np.zeros(M), np.where(np.arange(M) % 2, 1.5, -1.5), np.full(M, -5.0)], uni(), far, True))

    def tie(f, rnd):        # an exact tie between components 2 and 7 (same logit, same random: same float operations)
        assert np.all(f['gap'] == 0.0) and np.all(f['k'] == 2)
        assert np.all(rnd[..., 2] == rnd[..., 7])
    lg = np.full(M, -30.0)
    lg[[2, 7]] = 0.0        # the others cannot win: -30 - log(-log(1 - 1e-5)) = -18.5 < 0 - log(-log(1e-5)) = -2.4
    mt = np.zeros(M)
    mt[2], mt[7] = -0.5, 0.5        # 32768 index steps apart: the index tells which component was taken
    r = uni()
    r[..., 7] = r[..., 2]
    out.append(('argmax_tie', np.r_[lg, mt, np.full(M, -6.0)], r, tie, False))

    def ends(f, rnd):       # u at both ends of its range, selection and value draws
        assert rnd.min() == U_LO and rnd.max() == U_HI and np.all(np.abs(f['x_pre']) < 0.9)
    r = np.where(rs.uniform(0, 1, [Tn, B, M + 1]) < 0.5, U_LO, U_HI).astype(np.float32)
    out.append(('u_ends', np.r_[logits, means, np.full(M, -4.0)], r, ends, False))
    return out


def _gauss_edges(hp, B):
    Tn, Q = EDGE_TN, 65536
    rs = np.random.RandomState(12)
    out = []

    def low(f, rnd):
        assert f['ls_raw'] < -7.0
        assert (_index(f['x_unclamped'], Q) != _index(f['x_pre'], Q)).mean() > 0.5
    out.append(('log_std_-9', [0.3, -9.0], rs.standard_normal([Tn, B, 1]).astype(np.float32), low, False))

    def clip(f, rnd):
        assert np.all(np.abs(f['x_pre']) > 2.0) and (f['x_pre'] < 0).any() and (f['x_pre'] > 0).any()
    out.append(('z_+-40', [0.0, math.log(0.2)], np.where(rs.uniform(0, 1, [Tn, B, 1]) < 0.5, -40.0, 40.0).astype(np.float32),
                clip, True))

    def top(f, rnd):        # exactly the upper clip bound, 1 - 2/Q = 1 - 2^-15 (a float32)
        assert np.all(f['x_pre'] == 1.0 - 2.0 / Q) and np.float32(1.0 - 2.0 / Q) == 1.0 - 2.0 / Q
    out.append(('mean_at_top', [1.0 - 2.0 / Q, -3.0], np.zeros([Tn, B, 1], np.float32), top, True))
    return out


def _ce_edges(hp, B):
    Tn, n = EDGE_TN, 256
    rs = np.random.RandomState(13)
    row_full, row_zero = rs.uniform(-2, 2, n), rs.uniform(-2, 2, n)     # (rows first: they must not depend on B)
    u = rs.uniform(0, 1, [Tn, B, 1]).astype(np.float32)
    u[0::4] = 0.0                   # steps 0, 4, ...: u = 0; steps 1, 5, ...: the largest float32 below 1
    u[1::4] = F32_BELOW_1
    exact = (u[..., 0] == 0) | (u[..., 0] == F32_BELOW_1)
    out = []

    def full(f, rnd):
        assert np.all(f['k'][rnd[..., 0] == 0] == 0) and np.all(f['k'][rnd[..., 0] == F32_BELOW_1] == n - 1)
    out.append(('u_0_and_below_1', row_full, u, full, exact))

    def zero_mass(f, rnd):  # zero mass in float64 too: u = 0 skips the first 100 classes, u next to 1 stops at class 155
        assert np.all(f['e'][:100] == 0.0) and np.all(f['e'][-100:] == 0.0) and np.all(f['e'][100:156] > 1e-3)
        assert np.all(f['k'][rnd[..., 0] == 0] == 100) and np.all(f['k'][rnd[..., 0] == F32_BELOW_1] == 155)
        assert f['k'].min() >= 100 and f['k'].max() <= 155
    row = row_zero
    row[:100] = row[-100:] = -1000.0
    out.append(('zero_mass_classes', row, u, zero_mass, exact))

    def one_hot(f, rnd):
        assert np.all(f['k'] == 37)
    row = np.full(n, -1000.0)
    row[37] = 0.0
    out.append(('one_hot', row, u, one_hot, True))
    return out


def edge_cases(loss, B):
    """[(name, row [ow], rnd [EDGE_TN, B, n_rand], reached(facts, rnd), exact)] of one head: `reached` asserts on the float64
    sampler that the edge is met; `exact` (True, or a [Tn, B] mask) marks draws where float32 and float64 cannot differ (a
    clipped value, an exact zero of mass) and the index must EQUAL the float64 one, beyond the parity rule."""
    _, hp, _, _, _ = case(EDGE_GEOM, EDGE_HEADS[loss])
    return {'mol': _mol_edges, 'gauss': _gauss_edges, 'ce': _ce_edges}[loss](hp, B)


EDGE_IDS = [(loss, i) for loss, n in (('mol', 5), ('gauss', 3), ('ce', 3)) for i in range(n)]


def check_edge(tag, hp, edge, idx, out_params, wav=None):
    """What both the engine and the float32 oracle sampler are held to on an edge row: the edge is reached on the float64
    sampler, the parity rule, equality where `exact`, the tie rule, the index range and (wav given) the de-quantised feedback."""
    name, row, rnd, reached, exact = edge
    B, Tn = idx.shape
    Q = O.quant_chann_of(hp)
    row32 = np.asarray(row, np.float32)
    reached(sampler_facts(hp, row32, rnd), rnd)
    assert np.array_equal(out_params, np.broadcast_to(row32, out_params.shape)), name      # 0 * z + bias is exact
    assert idx.min() >= -Q // 2 and idx.max() < Q // 2
    assert_sampler_parity('{} {} B={}'.format(tag, name, B), hp, out_params, rnd, idx)
    p = sampler_parity(hp, out_params, rnd, idx)
    ex = np.broadcast_to(np.asarray(exact), (Tn, B)).T
    assert np.all(p['d'][ex] == 0), (name, 'differs from float64 where it cannot', int((p['d'][ex] != 0).sum()))
    if name == 'argmax_tie':        # the parity rule excuses any component at a tie; argmax takes the first: component 2
        assert np.all(np.abs(p['d']) <= 1) and np.all((p['d'] == 0) | (p['margin'] <= 0.02)), name
    if wav is not None:
        assert np.abs(wav - dequant(idx, hp)).max() <= 2.0 ** -23
    return p['n_flip']


# ---------------------------------------------------------------------------------------------------------------------
# 3. distribution of the draws on fixed network outputs; every bound is 5 standard errors computed from N
# ---------------------------------------------------------------------------------------------------------------------
STAT_TN = 2048
STAT_BATCHES = (16, 2)              # N = 32 768 and 4 096
STAT_SEED = 20261
STAT_HEADS = {'gauss': ('gauss', {}), 'mol': ('mol10', dict(mol_mix=3)), 'ce': ('ce', {})}
MOL3_P = np.array([0.5, 0.3, 0.2])
MOL3_MEANS = np.array([-0.5, 0.0, 0.5])
MOL3_SCALE = 0.01
STAT_ROWS = {
    'gauss': np.array([0.1, math.log(0.2)]),
    'mol': np.r_[np.log(MOL3_P), MOL3_MEANS, np.full(3, math.log(MOL3_SCALE))],
    'ce': np.log(1.0 + np.arange(256) % 7),
}


def stat_config(loss):
    head, patch = STAT_HEADS[loss]
    return dict(config(EDGE_GEOM, head), **patch)


def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def draw_statistics(loss, idx):
    """[(name, |statistic - target|, bound)] of the indices idx [B, Tn] drawn on STAT_ROWS[loss].  Q = 65536 for gauss / mol
    (wav = idx / 32768, the floor shifts the mean by half a step, 2^-16), 256 classes for ce."""
    B, Tn = idx.shape
    N = B * Tn
    out = []
    if loss == 'ce':
        v = idx.astype(np.float64)
        if N >= 32768:      # Pearson chi-square with 255 degrees of freedom: mean 255, variance 510
            p = np.exp(STAT_ROWS['ce'])
            p /= p.sum()
            cnt = np.bincount(idx.reshape(-1) + 128, minlength=256)
            out.append(('chi-square of the 256 class counts', float(((cnt - N * p) ** 2 / (N * p)).sum()), 255 + 5 * math.sqrt(510)))
    else:
        v = idx.astype(np.float64) / 32768.0
    if loss == 'gauss':
        out.append(('mean', abs(v.mean() - (0.1 - 2.0 ** -16)), 5 * 0.2 / math.sqrt(N)))
        out.append(('standard deviation', abs(v.std() - 0.2), 5 * 0.2 / math.sqrt(2 * N)))
    if loss == 'mol':
        k = np.abs(v[..., None] - MOL3_MEANS).argmin(axis=-1)           # nearest mean: 25 scales to the midpoint
        r = v + 2.0 ** -16 - MOL3_MEANS[k]
        for c in range(3):
            pc = MOL3_P[c]
            out.append(('frequency of component %d' % c, abs((k == c).mean() - pc), 5 * math.sqrt(pc * (1 - pc) / N)))
        var = (MOL3_SCALE * math.pi) ** 2 / 3                           # logistic: variance s^2 pi^2 / 3, kurtosis 4.2
        out.append(('pooled residual variance', abs((r * r).mean() - var), 5 * var * math.sqrt(3.2 / N)))
        out.append(('corr(component, sign of residual)', abs(_corr(k.astype(np.float64), np.sign(r))), 5 / math.sqrt(N)))
    out.append(('lag-1 autocorrelation along time', abs(_corr(v[:, :-1].reshape(-1), v[:, 1:].reshape(-1))), 5 / math.sqrt(B * (Tn - 1))))
    out.append(('corr(row 0, row 1)', abs(_corr(v[0], v[1])), 5 / math.sqrt(Tn)))
    return out


def assert_statistics(tag, loss, idx):
    stats = draw_statistics(loss, idx)
    for name, dev, bound in stats:
        print('{} N={}: {}: {:.4g} (bound {:.4g})'.format(tag, idx.size, name, dev, bound))
    for name, dev, bound in stats:
        assert dev < bound, (tag, name, dev, bound)
