"""The inverse of the IAF student on the CPU, built on oracle.wavenet_np.iaf_feed_forward.

feed_forward returns x = z * scale_tot(z) + mean_tot(z) with scale_tot[t], mean_tot[t] functions of z[<t] only, so
z <- (x - mean_tot(z)) / scale_tot(z) is a triangular fixed point: after k sweeps the first k samples are exact for the
dtype, after T sweeps the row.  Three things come from here:

  * the float64 inverse of an x that is the float64 forward of a known z0: z0 itself (`forward`);
  * the sweep loop in a chosen dtype (`inverse`): in float32 the yardstick an engine's own float32 sweeps are held to, in
    float64 the inverse of an x no z0 produced (an engine's float32 x, real audio);
  * the float64 log-density log p(x[t]) = log f(z[t]) - log scale_tot[t] (`log_density`), untruncated.

A helper, not a test module: tests/test_iaf_inverse_oracle.py holds it to these claims.
"""
import numpy as np

from oracle import wavenet_np as wn


def forward(mel, z, weights, hp, dtype=np.float64):
    """iaf_feed_forward with the noise injected: 'x', 'mean_tot', 'scale_tot', 'log_scale_tot' in `dtype`."""
    return wn.iaf_feed_forward(np.asarray(mel, dtype), np.asarray(z, dtype), weights, hp, dtype)


def sweep(mel, x, z, weights, hp, dtype=np.float64):
    """One sweep: (z', the forward at z).  z' = (x - mean_tot(z)) / scale_tot(z), all in `dtype`."""
    o = forward(mel, z, weights, hp, dtype)
    return (np.asarray(x, dtype) - o['mean_tot']) / o['scale_tot'], o


def inverse(mel, x, weights, hp, dtype=np.float64, z_init=None, max_sweeps=None, trace=None):
    """Sweeps from z_init (zeros) until a sweep changes no bit, at most max_sweeps (T).  Returns {'z', 'sweeps' (the
    sweeps run, the confirming one included), 'converged', 'mean_tot', 'scale_tot', 'log_scale_tot' (of the last sweep's
    input, which is z itself when converged)}.  trace: a list that receives every iterate."""
    x = np.asarray(x, dtype)
    T = x.shape[1]
    max_sweeps = T if max_sweeps is None else max_sweeps
    z = np.zeros_like(x) if z_init is None else np.array(z_init, dtype)
    o, n, same = None, 0, False
    while n < max_sweeps and not same:
        zn, o = sweep(mel, x, z, weights, hp, dtype)
        n += 1
        same = zn.tobytes() == z.tobytes()
        z = zn
        if trace is not None:
            trace.append(z.copy())
    return {'z': z, 'sweeps': n, 'converged': same, 'mean_tot': o['mean_tot'], 'scale_tot': o['scale_tot'],
            'log_scale_tot': o['log_scale_tot']}


def log_density(z, log_scale_tot, loss_type):
    """float64 log p(x[t]) = log f(z[t]) - log scale_tot[t]; f = Logistic(0,1) (-z - 2 softplus(-z)) for 'logistic',
    Normal(0,1) for 'gauss'.  The reference's clip of its uniform draw to [1e-5, 1 - 1e-5] is ignored."""
    z = np.asarray(z, np.float64)
    ls = np.asarray(log_scale_tot, np.float64)
    if loss_type == 'gauss':
        lf = -0.5 * z * z - 0.5 * np.log(2.0 * np.pi)
    else:
        lf = -z - 2.0 * (np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z))))
    return lf - ls


def latent_draw(loss_type, shape, seed=6):
    """z0 as the student draws it: logistic from u ~ U(1e-5, 1 - 1e-5), or normal; float64."""
    rs = np.random.RandomState(seed)
    if loss_type == 'gauss':
        return rs.standard_normal(shape)
    u = rs.uniform(1e-5, 1.0 - 1e-5, size=shape)
    return np.log(u) - np.log(1.0 - u)
