"""The TRAIN update (include/ssd_hip.h, block "the TRAIN update") restated in numpy: float32 op by op (what csrc/update.hip must
match bit for bit) and float64 (the yardstick of the float32 form).  Independent of the package: nothing is imported from it."""
import math

import numpy as np

F = np.float32


def learning_rate(config, global_step):
    n = config["num_steps"]
    return config["initial_learning_rate"] * 0.5 * (1.0 + math.cos(math.pi * min(global_step, n) / n))


def ema_decay(t):
    return min(0.993, (1.0 + t) / (10.0 + t))


def scalars(config, t, epsilon=1e-8, dtype=np.float32):
    """(alpha, 1 - beta1, 1 - beta2, epsilon, weight_decay, 1 - d) of update t = 1, 2, ...: float64 on the host, rounded once."""
    lr = float(F(learning_rate(config, t - 1)))
    alpha = lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
    return tuple(dtype(x) for x in (alpha, 0.1, 0.001, epsilon, config["weight_decay"], 1.0 - ema_decay(t)))


def decays(name):
    return ("weights" in name or "kernel" in name) and "depthwise_weights" not in name


def update(w, g, m, v, ema, decay, sc):
    """One update of one tensor, in place, in the dtype of the arrays (float32: one rounding per operation, as numpy does on arrays
    of one dtype with scalars of the same dtype).  g None: only ema moves."""
    alpha, omb1, omb2, eps, wd, omd = sc
    dt = w.dtype.type
    assert all(a.dtype == w.dtype for a in (m, v, ema)) and all(type(x) is dt for x in sc)
    if g is not None:
        assert g.dtype == w.dtype
        gp = g + wd * w if decay else g
        m += (gp - m) * omb1
        v += (gp * gp - v) * omb2
        w -= (m * alpha) / (np.sqrt(v) + eps)
    ema -= (ema - w) * omd


def run(config, tensors, grads_per_step, decay_flags, first_t=1, epsilon=1e-8):
    """tensors: list of [w, m, v, ema] arrays (updated in place); grads_per_step: one list of gradients (or None) per step."""
    dtype = tensors[0][0].dtype.type
    for k, grads in enumerate(grads_per_step):
        sc = scalars(config, first_t + k, epsilon, dtype)
        for (w, m, v, ema), g, d in zip(tensors, grads, decay_flags):
            update(w, g, m, v, ema, d, sc)
