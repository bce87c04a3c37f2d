"""Float64 oracle of the upsampler's reverse pass: the transposed-conv stack restated on torch's
conv_transpose1d with padding = (K - S) / 2, then the activation, so that torch.autograd gives the gradient of every
trans_conv_j/kernel and trans_conv_j/bias.  tests/test_deconv_grad_oracle.py pins it on the CPU (forward against
oracle.wavenet_np.deconv_stack, gradients against central differences); tests/test_gpu_deconv_backward.py holds the engine
to it.  Also the tie handling of leaky-relu, which works on this oracle alone: row seeds whose hidden pre-activations keep
clear of zero, and a mask of the last layer's near-zero pre-activations.  relu (masked.get_upsample_act's third name) goes
by the same tie rules on its pre-activations; an unknown name raises.  Stacks of any number of layers are served, except by
the projection of hidden ties, which stays two-layer.

pick_rows searches until it finds a clear seed.  One shape of the GPU tests has none in practice: a hidden tensor of 256
channels x 270 frames has 69 120 values, and a band of 1e-4 of the largest magnitude around zero catches 15 to 28 of them
for each of the seeds 2001 .. 2010 (a clear seed would be one in about e^20).  For that shape alone pick_rows_fewest takes
the seed of that window with the fewest near ties, the test asserts that no seed of the window is clear, and mask_last
removes from the cotangent its component along the few directions that reach those hidden elements (a projection
computed in float64 from the oracle's own weights), so that their cotangent is zero and the sign the engine takes there
cannot matter -- the same treatment the last layer gets, one layer down."""
import numpy as np
import torch
import torch.nn.functional as TF

BAND = 1e-4                 # a pre-activation within BAND * max |z| of zero is a near tie
FIRST_SEED = 2001
MAX_ZEROED = 1e-3           # at most 0.1 % of a case's cotangent may be zeroed
BATCH = 64                  # seeds evaluated at a time by the search for a clear row
SEARCH_LIMIT = 20000        # seeds after which the search gives up
WINDOW = 10                 # pick_rows_fewest: seeds looked at per row
MAX_HIDDEN = 64             # pick_rows_fewest: hidden near ties per row a case may project out


def names(n_layers, prefix=''):
    p = prefix + '/' if prefix else ''
    out = []
    for j in range(n_layers):
        out += ['{}trans_conv_{:d}/kernel'.format(p, j + 1), '{}trans_conv_{:d}/bias'.format(p, j + 1)]
    return out


def weights64(w, n_layers, prefix=''):
    return {k: torch.as_tensor(np.asarray(w[k], np.float64)) for k in names(n_layers, prefix)}


def activation(z, act):
    """masked.get_upsample_act on a float64 tensor; torch.relu has no gradient at exactly 0"""
    if act == 'leaky_relu':
        return TF.leaky_relu(z, 0.4)
    if act == 'relu':
        return torch.relu(z)
    if act == 'tanh':
        return torch.tanh(z)
    raise ValueError('Unsupported activation function for upsample layer: {!r}'.format(act))


def stack_ff(mel, w, deconv_config, act, prefix=''):
    """mel [B,F,n_mel] float64, w {name: float64 tensor, TF shapes} -> ([pre-activation z_j [B,C,T_j]], enc [B,TE,Cd]);
    a stack of any number of layers"""
    p = prefix + '/' if prefix else ''
    h = torch.as_tensor(mel, dtype=torch.float64).transpose(1, 2)
    pre = []
    for j, (fl, s) in enumerate(deconv_config):
        W, b = w['{}trans_conv_{:d}/kernel'.format(p, j + 1)], w['{}trans_conv_{:d}/bias'.format(p, j + 1)]
        assert W.shape[1] == fl and (fl - s) % 2 == 0
        z = TF.conv_transpose1d(h, W[0].permute(2, 1, 0).contiguous(), b, stride=s, padding=(fl - s) // 2)
        pre.append(z)
        h = activation(z, act)
    return pre, h.transpose(1, 2)


def grads(mel, w, deconv_config, act, g, prefix=''):
    """{name: d sum(enc * g) / d variable} in float64"""
    ks = names(len(deconv_config), prefix)
    leaves = {k: w[k].clone().requires_grad_(True) for k in ks}
    _, enc = stack_ff(mel, leaves, deconv_config, act, prefix)
    got = torch.autograd.grad((enc * torch.as_tensor(g, dtype=torch.float64)).sum(), [leaves[k] for k in ks])
    return dict(zip(ks, got))


def near(z):
    """boolean mask of the near ties of a pre-activation tensor [B,C,T]: within BAND of the row's largest magnitude of zero"""
    return z.abs() <= BAND * z.abs().amax(dim=(1, 2), keepdim=True)


def hidden_ties(mels, w, deconv_config, prefix='', act='leaky_relu'):
    """per row of mels [n,F,n_mel]: the number of near ties in the hidden layers (every layer but the last; none in a stack
    of one layer) under the activation `act` between them"""
    p = prefix + '/' if prefix else ''
    h = torch.as_tensor(mels, dtype=torch.float64).transpose(1, 2)
    n = torch.zeros(h.shape[0], dtype=torch.int64)
    for j, (fl, s) in enumerate(deconv_config[:-1]):
        W, b = w['{}trans_conv_{:d}/kernel'.format(p, j + 1)], w['{}trans_conv_{:d}/bias'.format(p, j + 1)]
        z = TF.conv_transpose1d(h, W[0].permute(2, 1, 0).contiguous(), b, stride=s, padding=(fl - s) // 2)
        n += near(z).sum(dim=(1, 2))
        h = activation(z, act)
    return n.tolist()


def _mel_row(seed, F, n_mel):
    return np.random.RandomState(seed).uniform(0, 1, [F, n_mel]).astype(np.float32)


def pick_rows(B, F, w, deconv_config, act, prefix='', n_mel=80):
    """(mel [B,F,n_mel] float32, seeds): row i is np.random.RandomState(seed).uniform(0, 1, [F, n_mel]) of the first seed from
    FIRST_SEED upward (after row i - 1's) whose hidden pre-activations have no near tie.  The search goes on until it finds
    one (SEARCH_LIMIT seeds at the most, then it fails).  leaky_relu and relu search; tanh has no ties: consecutive seeds"""
    activation(torch.zeros(1, dtype=torch.float64), act)          # raises on an unknown name
    if act == 'tanh':
        seeds = tuple(range(FIRST_SEED, FIRST_SEED + B))
        return np.stack([_mel_row(s, F, n_mel) for s in seeds]), seeds
    rows, seeds, seed = [], [], FIRST_SEED
    while len(rows) < B:
        assert seed < FIRST_SEED + SEARCH_LIMIT, 'no seed without a hidden near tie'
        cand = list(range(seed, seed + BATCH))
        mels = np.stack([_mel_row(s, F, n_mel) for s in cand])
        ties = hidden_ties(mels, w, deconv_config, prefix, act)
        clear = [i for i, n in enumerate(ties) if n == 0]
        if not clear:
            seed += BATCH
            continue
        rows.append(mels[clear[0]])
        seeds.append(cand[clear[0]])
        seed = cand[clear[0]] + 1
    return np.stack(rows), tuple(seeds)


def pick_rows_fewest(B, F, w, deconv_config, prefix='', n_mel=80):
    """For the one shape where the rule of pick_rows has no answer: (mel, seeds, tie counts of the whole window).  Row i is
    the seed with the fewest hidden near ties of the WINDOW seeds after row i - 1's (from FIRST_SEED); the caller asserts
    that no seed of the window is clear, and mask_last projects the ties out of the cotangent"""
    rows, seeds, counts, seed = [], [], [], FIRST_SEED
    for _ in range(B):
        cand = list(range(seed, seed + WINDOW))
        mels = np.stack([_mel_row(s, F, n_mel) for s in cand])
        ties = hidden_ties(mels, w, deconv_config, prefix)
        best = min(range(WINDOW), key=lambda i: (ties[i], i))
        assert ties[best] <= MAX_HIDDEN, ties
        rows.append(mels[best])
        seeds.append(cand[best])
        counts.append(tuple(ties))
        seed = cand[best] + 1
    return np.stack(rows), tuple(seeds), tuple(counts)


def _project_hidden(g, keep, pre, w, deconv_config, prefix):
    """g [B,TE,Cd] float64 minus its component along d enc / d h[b,c,f] of every hidden near tie (b,c,f), inside `keep`"""
    assert len(deconv_config) == 2, 'hidden ties are projected out for two-layer stacks'
    p = prefix + '/' if prefix else ''
    fl, s = deconv_config[1]
    w2 = w['{}trans_conv_2/kernel'.format(p)][0].permute(2, 1, 0).contiguous()           # [Cin,Cout,K]
    act2 = torch.where(pre[1] > 0, 1.0, 0.4).double()                                     # [B,Cout,T]
    ties = near(pre[0])
    g = g.clone()
    total = 0
    for b in range(g.shape[0]):
        idx = ties[b].nonzero()
        if len(idx) == 0:
            continue
        total += len(idx)
        rows = []
        for c, f in idx.tolist():
            one = torch.zeros((1,) + tuple(pre[0].shape[1:]), dtype=torch.float64)
            one[0, c, f] = 1.0
            j = TF.conv_transpose1d(one, w2, None, stride=s, padding=(fl - s) // 2)[0] * act2[b]    # d enc[b] / d h[b,c,f]
            rows.append((j.transpose(0, 1) * keep[b]).reshape(-1))
        A = torch.stack(rows)
        gb = g[b].reshape(-1)
        gb -= A.t() @ torch.linalg.solve(A @ A.t(), A @ gb)
        assert float((A @ gb).abs().max()) <= 1e-9 * float(gb.abs().max())
    return g, total


def mask_last(g, mel, w, deconv_config, act, prefix='', project=False):
    """g [B,TE,Cd] with the elements at near ties of the LAST layer's pre-activation set to zero -> (g float32, number zeroed,
    hidden ties).  Asserts that the zeroed share is within MAX_ZEROED and that no hidden layer has a near tie -- unless
    project=True (rows of pick_rows_fewest): then g also loses its component that reaches a hidden near tie"""
    if act == 'tanh':
        return g, 0, 0
    assert act == 'leaky_relu' or not project, 'hidden ties are projected out under leaky-relu only'
    pre, _ = stack_ff(mel, w, deconv_config, act, prefix)
    m = near(pre[-1]).transpose(1, 2)
    n = int(m.sum())
    assert n <= MAX_ZEROED * m.numel(), (n, m.numel())
    g = g.clone()
    g[m] = 0
    nh = sum(int(near(z).sum()) for z in pre[:-1])
    assert project or nh == 0, 'a hidden pre-activation is a near tie'
    if nh:
        g64, nh = _project_hidden(g.double(), (~m).double(), pre, w, deconv_config, prefix)
        g = g64.float()
        assert int((g[m] != 0).sum()) == 0
    return g, n, nh
