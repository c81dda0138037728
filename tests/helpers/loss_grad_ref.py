"""The gradient of the EVAL loss with respect to the head outputs, in float64, written out by hand on top of
loss_ref.training_targets (include/ssd_hip.h, ssd_loss_backward): the same formulas, in the same order, as the kernel, so
that rounding the result to float32 gives the kernel's value within one ulp (the kernel's exp / log1p are the device's
double ones).  Test infrastructure only."""
import numpy as np

from . import loss_ref

f32 = np.float32


def focal_grad(x, z, gamma=2.0, alpha=0.25):
    """d focal / dx element-wise in float64 (before g / norm): x float32 logits, z bool one-hot of the target class."""
    x = np.asarray(x, f32).astype(np.float64)
    z = np.asarray(z, bool)
    e = np.exp(-np.abs(x))
    r = 1.0 / (1.0 + e)
    s = np.where(x >= 0, r, e * r)                       # sigma(x)
    sc = np.where(x >= 0, e * r, r)                      # 1 - sigma(x), without cancellation
    nlp = (np.maximum(x, 0.0) - np.where(z, x, 0.0)) + np.log1p(e)
    q = np.where(z, sc, s)
    dq = np.where(z, -(s * sc), s * sc)
    smz = np.where(z, -sc, s)
    g = float(f32(gamma))
    if g == 2.0:
        t1 = 2.0 * q * dq * nlp
        qg = q * q
    else:
        qg = np.power(q, g)
        t1 = g * qg * np.where(z, -s, sc) * nlp            # dq/dx = +-q(1-q) folded into q^(gamma-1): 0 at q == 0
    aw = np.where(z, float(f32(alpha)), float(f32(1.0 - alpha)))
    return aw * (t1 + qg * smz)


def smooth_l1_grad(codes, targets):
    """d smooth-L1 / d codes element-wise (before g / norm): diff one float32 op, sign(diff) at |diff| >= 1."""
    d = np.asarray(codes, f32) - np.asarray(targets, f32)
    return np.where(np.abs(d) < f32(1), d, np.sign(d)).astype(np.float64)


def batch_grads(logits, codes, anchors, boxes, labels, num, gamma=2.0, alpha=0.25, grad=(1.0, 1.0), pos=0.5, neg=0.5):
    """d (localization_loss, classification_loss) . grad / d (logits [B,N,C], codes [B,N,4]) in float64 (the kernel's
    value before its one rounding to float32); norm = max(matches over the batch, 1) in float32, as ssd_loss forms it."""
    B, N, C = np.shape(logits)
    targets = []
    total = 0
    for b in range(B):
        n = int(num[b])
        reg, cls, m = loss_ref.training_targets(anchors, boxes[b][:n], labels[b][:n], pos, neg)
        targets.append((reg, cls, m))
        total += int((m >= 0).sum())
    norm = float(max(f32(total), f32(1)))
    gl = float(f32(grad[0])) / norm
    gc = float(f32(grad[1])) / norm
    d_logits = np.zeros((B, N, C), np.float64)
    d_codes = np.zeros((B, N, 4), np.float64)
    for b, (reg, cls, m) in enumerate(targets):
        z = cls[:, None] == np.arange(1, C + 1)[None, :]
        d_logits[b] = np.where((m >= -1)[:, None], focal_grad(logits[b], z, gamma, alpha) * gc, 0.0)
        d_codes[b] = np.where((m >= 0)[:, None], smooth_l1_grad(codes[b], reg) * gl, 0.0)
    return d_logits, d_codes
