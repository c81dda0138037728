"""The TRAIN FPN's references (include/ssd_hip.h, "the TRAIN FPN"): helpers.train_ops_ref's convolution (re-exported here), the
float32 restatement of ssd_fpn_merge_backward's line, and fpn() (feature_extractor.py:40-76) in torch on the CPU in a chosen
dtype with autograd."""
import numpy as np

from helpers import head_train_ref as href
from helpers.train_ops_ref import conv, conv_grads, dilate, integer_premise, out_hw, rows_per_slice, wgrad_bound   # noqa: F401

f32 = np.float32
EPS, MOMENTUM = href.EPS, href.MOMENTUM


def merge_f32(g, base=None, gate=None, same_size=False):
    """ssd_fpn_merge_backward's line in numpy float32, left to right."""
    g = g.astype(f32)
    terms = [g] if same_size else [g[:, 0::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 0::2], g[:, 1::2, 1::2]]
    acc = np.zeros(terms[0].shape, f32) if base is None else base.astype(f32).copy()
    with np.errstate(invalid="ignore"):
        opened = np.ones(acc.shape, bool) if gate is None else (gate.astype(f32) > 0)
    for t in terms:
        acc = (acc + np.where(opened, t, f32(0))).astype(f32)
    return acc


# ----------------------------------------------------------------------------- fpn() in torch on the CPU
KERNELS = ["fpn/lateral3/kernel", "fpn/lateral4/kernel", "fpn/lateral5/kernel"] + ["fpn/p%d/kernel" % i for i in range(3, 8)]


def torch_fpn(W, feats, dtype, training=True):
    """fpn() written from feature_extractor.py:40-76 in torch ops of `dtype` on the CPU, batch statistics in training mode.
    W {name: array} (fpn/* read), feats [c3, c4, c5] NHWC numpy.  -> ([p3 .. p7] NHWC tensors, T {name: leaf tensor of every
    trainable variable}, S {name: updated moving statistic as a tensor}, gates: the raw p6 as a tensor)."""
    import torch
    import torch.nn.functional as F
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in W.items()
         if k.startswith("fpn/") and k.rsplit("/", 1)[1] in ("kernel", "gamma", "beta")}
    c = {i: torch.tensor(f.astype(np.float64), dtype=dtype).permute(0, 3, 1, 2) for i, f in zip((3, 4, 5), feats)}

    def conv2d_same(x, name, stride=1):                                   # layer_utils.py:15-43
        w = T["fpn/%s/kernel" % name].permute(3, 2, 0, 1)
        k = w.shape[2]
        if stride == 1:
            return F.conv2d(x, w, padding=(k - 1) // 2)
        return F.conv2d(F.pad(x, (1, 1, 1, 1)), w, stride=stride)
    up = lambda x: x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    x = conv2d_same(c[5], "lateral5")
    raw = {5: conv2d_same(x, "p5"), 6: conv2d_same(c[5], "p6", 2)}
    raw[7] = conv2d_same(torch.relu(raw[6]), "p7", 2)
    for i in (4, 3):
        x = up(x) + conv2d_same(c[i], "lateral%d" % i)
        raw[i] = conv2d_same(x, "p%d" % i)
    outs, S = [], {}
    omm = float(f32(1.0 - MOMENTUM)) if dtype == torch.float32 else 1.0 - MOMENTUM
    for i in range(3, 8):
        s = "fpn/p%d_batch_norm" % i
        v = raw[i]
        g, b = T[s + "/gamma"].view(1, -1, 1, 1), T[s + "/beta"].view(1, -1, 1, 1)
        mm = torch.tensor(np.asarray(W[s + "/moving_mean"], np.float64), dtype=dtype)
        mv = torch.tensor(np.asarray(W[s + "/moving_variance"], np.float64), dtype=dtype)
        if training:
            mean = v.mean((0, 2, 3))
            var = ((v - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            rows = v.numel() // v.shape[1]
            unb = rows / (rows - 1.0) if rows > 1 else 1.0
            S[s + "/moving_mean"] = (mm - (mm - mean.detach()) * omm)
            S[s + "/moving_variance"] = (mv - (mv - var.detach() * unb) * omm)
        else:
            mean, var = mm, mv
        y = (v - mean.view(1, -1, 1, 1)) * (g / torch.sqrt(var.view(1, -1, 1, 1) + EPS)) + b
        outs.append(torch.relu(y).permute(0, 2, 3, 1))
    return outs, T, S, raw[6]


rel = href.rel
