"""Float64 numpy restatement of the TRAIN FPN's convolutions (include/ssd_hip.h, "the TRAIN FPN"): k = 1 or 3, stride 1 or 2 with
conv2d_same's explicit pad, their gradients, the zero-dilated form of the stride-2 data gradient, the float32 restatement of
ssd_fpn_merge_backward's line, and fpn() (feature_extractor.py:40-76) in torch on the CPU in a chosen dtype with autograd."""
import numpy as np

from helpers import head_train_ref as href

f32 = np.float32
EPS, MOMENTUM = href.EPS, href.MOMENTUM


def out_hw(H, W, stride):
    return -(-H // stride), -(-W // stride)


def _tap(x, kh, kw, k, stride):
    """x [B,H,W,C] -> what tap (kh,kw) reads per output position: x[b, oy*stride + kh - pad, ox*stride + kw - pad], zero outside."""
    B, H, W, C = x.shape
    pad = (k - 1) // 2
    OH, OW = out_hw(H, W, stride)
    p = np.zeros((B, H + 2 * pad + stride, W + 2 * pad + stride, C), x.dtype)
    p[:, pad:pad + H, pad:pad + W] = x
    return p[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]


def conv(x, w, stride=1, up=None):
    k = w.shape[0]
    x, w = x.astype(np.float64), w.astype(np.float64)
    y = 0.0
    for kh in range(k):
        for kw in range(k):
            y = y + _tap(x, kh, kw, k, stride) @ w[kh, kw]
    if up is not None:
        y = y + np.repeat(np.repeat(up.astype(np.float64), 2, axis=1), 2, axis=2)
    return y


def conv_grads(xs, w, dys, stride=1, absolute=False):
    """-> ([dx per level], dw) in float64; absolute=True: dw = the sums of |x * dy| per element."""
    k = w.shape[0]
    pad = (k - 1) // 2
    w64 = w.astype(np.float64)
    dw = np.zeros(w.shape, np.float64)
    dxs = []
    for x, dy in zip(xs, dys):
        x, dy = x.astype(np.float64), dy.astype(np.float64)
        B, H, W, C = x.shape
        OH, OW = dy.shape[1:3]
        buf = np.zeros((B, H + 2 * pad + stride, W + 2 * pad + stride, C), np.float64)
        for kh in range(k):
            for kw in range(k):
                a2, d2 = _tap(x, kh, kw, k, stride).reshape(-1, C), dy.reshape(-1, dy.shape[3])
                dw[kh, kw] += np.abs(a2).T @ np.abs(d2) if absolute else a2.T @ d2
                buf[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride] += dy @ w64[kh, kw].T
        dxs.append(buf[:, pad:pad + H, pad:pad + W])
    return dxs, dw


def dilate(dy, H, W):
    """D [B,H,W,C]: D[b,2oy,2ox] = dy[b,oy,ox], zero elsewhere (the stride-2 data gradient is conv3x3_same(D, w'))."""
    D = np.zeros((dy.shape[0], H, W, dy.shape[3]), dy.dtype)
    D[:, ::2, ::2] = dy
    return D


def integer_premise(xs, w, dys, stride):
    """-> (dw64, the largest sum of |x * dy| of a dw element): below 2^24 every partial sum of integers is exact in float32 in ANY order."""
    _, dw64 = conv_grads(xs, w, dys, stride)
    _, absum = conv_grads(xs, w, dys, stride, absolute=True)
    return dw64, float(absum.max())


def wgrad_bound(xs, w, dys, stride):
    """head_train_ref.wgrad_bound's derivation with n = the number of products of an element (output positions whose tap lies
    inside the input): |dw - dw64| <= gamma_n * sum|x * dy|, gamma_n = n u / (1 - n u), u = 2^-24, for ANY order of float32
    accumulation of exact products.  -> (dw64, bound, absum)"""
    _, dw64 = conv_grads(xs, w, dys, stride)
    _, absum = conv_grads(xs, w, dys, stride, absolute=True)
    _, n = conv_grads([np.ones(x.shape) for x in xs], w, [np.ones(d.shape) for d in dys], stride)
    u = 2.0 ** -24
    return dw64, n * u / (1 - n * u) * absum, absum


def rows_per_slice(out_rows, Cin, Cout, k):
    """include/ssd_hip.h's K-slice of the weight gradient: the TRAIN head's rule with 9 replaced by k * k, over OUTPUT rows."""
    tiles = k * k * (-(-Cin // 128)) * (-(-Cout // (32 if Cout <= 32 else 128)))
    want = max(1, 1536 // tiles)
    return -(-max(256, -(-sum(out_rows) // want)) // 16) * 16


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
