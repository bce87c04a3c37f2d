"""Float64 numpy restatement of what train_wavenet.py puts on top of the gradient: TensorFlow's Adam
(tf.train.AdamOptimizer: epsilon OUTSIDE the square root, the bias corrections folded into lr_t), tf.clip_by_global_norm
and tf.train.ExponentialMovingAverage with num_updates.  tests/test_adam_oracle.py pins it; tests/test_gpu_train_step.py
compares the kernels with it."""
import numpy as np


def lr_t(lr, beta1, beta2, t):
    """lr sqrt(1 - beta2^t) / (1 - beta1^t), t = 1 for the first step"""
    return float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t)


def clip_factor(sumsq, clip_norm):
    """tf.clip_by_global_norm scales every gradient by clip_norm / max(global_norm, clip_norm)"""
    return float(clip_norm) / max(np.sqrt(float(sumsq)), float(clip_norm))


def ema_decay(decay, num_updates):
    """tf.train.ExponentialMovingAverage(decay, num_updates): min(decay, (1 + n) / (10 + n))"""
    return min(float(decay), (1.0 + num_updates) / (10.0 + num_updates))


def adam_ema_step(p, g, m, v, ema, lr_t_, beta1, beta2, eps, ema_decay_t, sumsq=None, clip_norm=None):
    """One step from float64 copies of the state: returns {'p', 'm', 'v', 'ema' (None without a shadow), 'u' (the update
    subtracted from p), 'g' (the gradient after the clip)}.  Every scalar is taken as given (the GPU test hands over the
    float32 values the kernel receives)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gh = g * clip_factor(sumsq, clip_norm) if sumsq is not None else g
    b1, b2 = float(beta1), float(beta2)
    m1 = b1 * m + (1.0 - b1) * gh
    v1 = b2 * v + (1.0 - b2) * gh * gh
    u = float(lr_t_) * m1 / (np.sqrt(v1) + float(eps))
    p1 = p - u
    e1 = None
    if ema is not None:
        e = np.asarray(ema, np.float64)
        e1 = e - (1.0 - float(ema_decay_t)) * (e - p1)
    return {'p': p1, 'm': m1, 'v': v1, 'ema': e1, 'u': u, 'g': gh}
